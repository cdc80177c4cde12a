"""The precision watch: `--precision auto` picks a fast mode once, and every render loop keeps checking that choice the same way --
spot-check a sample of what was just rendered, agree between the ranks (dist.any_rank: one MAX all-reduce of one int), on a miss
anywhere step every rank one rung down, record the fallback, log one line, render again and check again.  Watch.run is that loop,
once; frontend.render_path (the teacher per frame, the student per batch), create_data.create_rand (per save group) and
online.OnlineTeacherSource.batch (per step) say how to check, how to step down and what to render again."""


class Watch:
    """The counters of one watched loop and the loop itself.  max_steps: how often one call checks at most (the teacher's loops:
    len(engine.LADDER)); log: takes the lines of the fallbacks; device: where any_rank's int lives under nccl; worst: {} keeps the
    maximum per key of checks that report a dict, 0.0 the maximum of checks that report one number."""

    def __init__(self, max_steps, log=None, device=None, worst=None):
        self.max_steps, self.log, self.device = int(max_steps), log, device
        self.checks, self.fallbacks, self.worst = 0, [], {} if worst is None else worst

    def stats(self):
        return {'checks': self.checks, 'fallbacks': self.fallbacks, 'worst': self.worst}

    def run(self, got, check, step_down, again, live=None, agree=None):
        """got: what was just rendered; returns what is to be handed on (got, or the last again()).
        check(got) -> (ok, differences), or None when this rank has nothing to check: good, and not counted.
        step_down(ok, differences) -> (the fallback's record, its log line or None): moves the engine one rung down; ok and differences
            are this rank's own (True, None without a check), so a rank that follows a peer can say so.
        again() -> the same render in the new mode.
        live() -> False: the engine has no fast mode left; leave before the check and the collective (all ranks share the mode).
        agree(flag) -> True when any rank says so: every rank calls it once per check, whatever it checked; default dist.any_rank
            over all ranks."""
        if agree is None:
            from .dist import any_rank
            agree = lambda flag: any_rank(flag, self.device)
        for _ in range(self.max_steps):
            if live is not None and not live():
                break
            verdict = check(got)
            ok, d = (True, None) if verdict is None else verdict
            if verdict is not None:
                self.checks += 1
                if isinstance(d, dict):
                    for k, v in d.items():
                        self.worst[k] = max(self.worst.get(k, 0.), v)
                else:
                    self.worst = max(self.worst, d)
            if not agree(not ok):
                break
            record, line = step_down(ok, d)
            self.fallbacks.append(record)
            if line is not None and self.log is not None:
                self.log(line)
            got = again()
        return got
