/*
 * r2l_hip.h — C-ABI of the MI355X (gfx950) renderer for the R2L / NeRF-teacher
 * ray-batched inference path of MingSun-Tse/Efficient-NeRF.
 *
 * The reference has no FFI: its hot path is ordinary Python calls on module-level
 * globals.  Each entry point below replaces one of those call sites (cited as
 * reference file:line).  All pointers are plain host or device pointers, sizes are
 * plain ints, streams are a `hipStream_t` passed as `void*` (0 = default stream).
 * No torch types cross this boundary.
 *
 * Conventions
 *   - every function returns 0 on success, a negative R2L_E* code otherwise;
 *     r2l_last_error() returns a thread-local message for the last failure.
 *   - "dev" pointers are device memory owned by the caller (a PyTorch-ROCm tensor's
 *     data_ptr()); the library borrows them for the duration of the stream-ordered
 *     call and never synchronises the stream.
 *   - weights are copied / re-packed once into library-owned device memory by the
 *     *_load_weights calls; tensors are float32, row-major `[out, in]` exactly as in
 *     the reference's `state_dict` (nn.Linear convention).
 *   - a context is not re-entrant across threads; use one context per stream.
 */
#ifndef R2L_HIP_H
#define R2L_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define R2L_OK 0
#define R2L_EINVAL -1   /* bad argument / unsupported configuration */
#define R2L_EHIP -2     /* a HIP runtime call failed (see r2l_last_error) */
#define R2L_ESTATE -3   /* call order violated (e.g. render before load_weights) */
#define R2L_ENOGPU -4   /* no gfx950 device visible */

/* precision_mode of the ResMLP / teacher MLP contractions (MFMA fp16 operands,
 * fp32 accumulate):
 *   R2L_PREC_FP16X3  hi/lo split of both operands, 3 MFMA passes per k-step
 *                    (ah*wh + ah*wl + al*wh): L_inf vs the fp32 reference ~1e-6;
 *   R2L_PREC_FP16X1  single pass on fp16-rounded operands, 3x fewer MFMAs.  R2L student: L_inf ~4e-4, outside the contract
 *                    (compiler-scheduled kernel, kept for reference).  NeRF teacher: 0.6-1.6e-5 on rgb over whole frames
 *                    (eleven layers, compositing over 192 samples) -- its FAST mode since round 4: the generated layer chain
 *                    without correction terms (nerf_chain_kernel<true, 4>: four 16-point column tiles per wave, embedding k-steps
 *                    hi / lo on the embedding side; since round 5 one statement that also loads its rays, computes the next tile's
 *                    embedding under the MFMAs and stores raw: nerf_chain_emb_kernel), 0.58-0.60 of the fp16 MFMA peak.  For SMOOTH
 *                    teachers only: on a trained one (sharp densities) it is 3e-3 .. 3e-1 off; the front end's `--precision auto`
 *                    measures it against FP16X3 on several poses per checkpoint and watches it afterwards.
 *   R2L_PREC_FP16_FP8  fp16 main pass + the two correction terms of FP16X3 on the block-scaled
 *                    low-precision MFMA (v_mfma_scale_f32_*_f8f6f4) with both operands in OCP bf6 (e3m2)
 *                    at 4x the fp16 rate: 1.5 pass-equivalents per k-step, L_inf ~3e-5 (< 1e-4).
 *                    R2L: generated head launch -> generated body kernel (32x32 shapes) -> tail launch;
 *                    teacher: generated layer chain (16x16 shapes; the embedding k-steps stay three
 *                    fp16 passes).  (The name is historical: round 1 used fp8 terms.) */
/*   R2L_PREC_FP16_E4M3 (R2L student only) the same machine with both correction terms in OCP e4m3 (3 mantissa bits instead
 *                    of 2 in all four factors): 2.0 pass-equivalents per k-step, half the error of R2L_PREC_FP16_FP8 -- the
 *                    mode for networks whose residual stream is too large for the bf6 terms (activation exponent 4:
 *                    `--precision auto` picks per checkpoint: FP16_FP8 up to exponent 3, FP16_E4M3 at 4, FP16X3 above). */
#define R2L_PREC_FP16X3 0
#define R2L_PREC_FP16X1 1
#define R2L_PREC_FP16_FP8 2
#define R2L_PREC_FP16_E4M3 3
/*   R2L_PREC_FP16X3_ASM FP16X3's arithmetic (hi/lo split of both operands, three fp16 MFMA passes per k-step) on the generated
 *                    kernels: no low-precision term anywhere, hence no operand scales, no calibration and nothing to watch.
 *                    R2L student: generated head and body kernels, L_inf 5-7e-7 against the reference's output, 7 % faster than the
 *                    compiler-scheduled FP16X3; the last rung of the front end's `--precision auto` (networks whose activations
 *                    are beyond FP16_E4M3's reach: e.g. the trained-like fixture, max|a| 126).  NeRF teacher (round 5): the
 *                    generated layer chain in three passes (nerf_chain_kernel<false, 2, true>; W x 2^k streamed as hi and lo
 *                    fragments), raw within 1.5e-5 of FP16X3, 17 % faster; `auto`'s last rung -- where every trained teacher ends. */
#define R2L_PREC_FP16X3_ASM 4
/*   R2L_PREC_FP16_SPLIT (R2L student only, round 5) for networks the activation limits send past FP16_FP8 / FP16_E4M3 (every
 *                    trained one so far: max|a| 126 on the trained-like fixture).  Measured on that network, rendered against three
 *                    passes everywhere: the bf6-term head launch alone costs 9e-5 of the 1e-4 contract, and of the body blocks the
 *                    EARLY ones cost most (their error is amplified by everything behind them).  So: head launch and blocks
 *                    [0, split) in FP16X3_ASM's arithmetic (three fp16 passes), blocks [split, n_block) in FP16_FP8's (generated
 *                    bf6 body kernel, 1.5 pass-equivalents, calibrated and range-guarded as in that mode); two body launches
 *                    hand the x image over (bit-exact: both kernels keep the stream in fp32).  r2l_set_split_block sets the split
 *                    (default n_block / 2); the front end's `--precision auto` measures the smallest split whose frame stays
 *                    inside its limit against three passes on every ray of a probe frame, and watches it.  split = n_block:
 *                    FP16X3_ASM's results bit for bit; split = 0: every body block with bf6 terms behind the three-pass head. */
#define R2L_PREC_FP16_SPLIT 5
/*   R2L_PREC_FP16_SPLIT8 the same two-part form with FP16_E4M3's arithmetic behind the split (e4m3 correction terms: 2.0
 *                    pass-equivalents, 0.44 x the error of the bf6 terms on the trained-like student).  Which of the two is cheaper at
 *                    the same error depends on the network -- the trained-like fixture: SPLIT8 at split 0 (11.3 ms per 800 x 800
 *                    frame) against SPLIT at split 21 (12.5 ms); its second variant: SPLIT at split 9 (10.9 ms) -- so `auto` bisects
 *                    both and takes the cheaper. */
#define R2L_PREC_FP16_SPLIT8 6
/*   R2L_PREC_FP16_MIX (NeRF teacher only, round 6) R2L_PREC_FP16_FP8's layer chain with its first two 256 x 256 trunk layers
 *                    (pts_linears.1, .2: model/nerf_raybased.py:379-386) in FP16X3_ASM's three fp16 passes and everything behind them
 *                    with bf6 correction terms: ~2.0 pass-equivalents.  For the FINE network of trained teachers (nerf_set_precision_pair
 *                    (FP16X3_ASM, FP16_MIX)): the sharp density tail of such a network amplifies the early layers' error, and with them
 *                    exact the fine pass stays within 3-4e-5 of three passes everywhere at fixed sample positions; the coarse network,
 *                    which steers sample_pdf, keeps FP16X3_ASM.  `--precision auto` measures it per checkpoint and watches it. */
#define R2L_PREC_FP16_MIX 7

typedef struct r2l_ctx r2l_ctx;
typedef struct nerf_ctx nerf_ctx;

const char* r2l_last_error(void);
/* number of visible HIP devices whose arch is gfx950 (0 => every call fails loudly) */
int r2l_device_count(void);

/* ---------------------------------------------------------------------------------
 * Multi-GPU: one process per GPU, the rows of a frame split contiguously over the ranks (rank r renders rows
 * [r*H/G + min(r, H%G), ...), the first H % G ranks one row more: r2l_render(..., row_begin, row_end, ...)),
 * ONE RCCL collective over xGMI assembles the frames on every rank.  The reference has no counterpart (it
 * renders on one GPU, main.py:473): SURVEY.md 8(b) seam 3 is the contract.  RCCL is bound at run time; a
 * process that never calls these needs no librccl.
 *   r2l_comm_available   0 when this process can bind RCCL (no id is made, no bootstrap socket opened: the pre-flight
 *                        of the ranks other than 0), else the code and message r2l_comm_create would fail with
 *   r2l_comm_unique_id   rank 0 obtains the 128-byte id and hands it to the other ranks by any host channel
 *   r2l_comm_create      every rank, after hipSetDevice(its GPU): ncclCommInitRank
 *   r2l_gather_image     local_rows_dev [n_frames, rows_of_this_rank * row_floats] -> full_image_dev
 *                        [n_frames, H * row_floats] on every rank (row_floats = W * 3 for RGB), stream-ordered;
 *                        one grouped launch: ncclAllGather per frame (equal shards) or ncclBroadcast per shard
 * --------------------------------------------------------------------------------- */
typedef struct r2l_comm r2l_comm;
int r2l_comm_available(void);
int r2l_comm_unique_id(char* id_out128);
int r2l_comm_create(r2l_comm** out, int rank, int world, const char* id128);
void r2l_comm_destroy(r2l_comm* comm);
int r2l_gather_image(r2l_comm* comm, const float* local_rows_dev, float* full_image_dev, int n_frames, int H,
                     int row_floats, void* stream);

/* ---------------------------------------------------------------------------------
 * R2L student (neural light field).  Replaces, under torch.no_grad():
 *   PointSampler.__init__            model/nerf_raybased.py:78-92   -> r2l_create
 *   NeRF_v3_2.__init__ + load        model/nerf_raybased.py:483-537,
 *                                    main.py:482-502                -> r2l_load_weights
 *   model(positional_embedder(point_sampler.sample_test(c2w)))
 *                                    main.py:300-309, 401-404       -> r2l_render
 *   model(positional_embedder(point_sampler.sample_train(o,d,0)))
 *                                    main.py:220-230                -> r2l_render_rays
 *   point_sampler.sample_test / positional_embedder alone
 *                                    model/nerf_raybased.py:94-102,198-208
 *                                                                   -> r2l_sample_embed
 * --------------------------------------------------------------------------------- */

/* H, W, focal: image geometry (focal as the Python float the reference passes, it is
 * rounded to f32 where the reference's tensor ops round it).  n_sample must be 16,
 * L (multires) 10 and width (netwidth) 256 — the R2L W256 family; n_block is the number
 * of ResMLP blocks ((netdepth-2)/2 = 43 for D88), any value >= 0.  use_residual = the
 * --use_residual global skip. */
int r2l_create(r2l_ctx** out, int H, int W, double focal, float near_, float far_,
               int n_sample, int L, int width, int n_block, int use_residual,
               int precision_mode);
void r2l_destroy(r2l_ctx* ctx);

/* tensors: 4 + 4*n_block HOST pointers in state_dict order:
 *   head.0.weight[256,1008], head.0.bias[256],
 *   body.{i}.body.0.weight[256,256], .bias[256], body.{i}.body.2.weight, .bias  (i < n_block),
 *   tail.0.weight[3,256], tail.0.bias[3]
 * May be called again on a live context.  A load that is refused (weights the current mode cannot pack, a NULL tensor) leaves the
 * context unloaded: renders and r2l_set_act_exponents return R2L_ESTATE until a load succeeds.  A HIP graph captured before a
 * reload holds pointers to the freed weight images; replaying it afterwards is the caller's error.                             */
int r2l_load_weights(r2l_ctx* ctx, const float* const* tensors, int n_tensors);
int r2l_set_precision(r2l_ctx* ctx, int precision_mode);
/* R2L_PREC_FP16_SPLIT / _SPLIT8: the number of leading blocks in three passes = first block of the bf6 / e4m3 part, 0 .. n_block (takes
 * effect at the next render; no re-packing) */
int r2l_set_split_block(r2l_ctx* ctx, int split_block);
/* Activations of NeRF_v3_2 / ResMLP other than the README's (model/nerf_raybased.py:443-476, 497-522: args.act behind the head layer,
 * trial.inact inside a block, trial.outact behind it), as slopes s of act(v) = max(v, s v): 0 = ReLU, 0.01 = LeakyReLU (torch's
 * default negative_slope), 1 = none.  Defaults 0, 0, 1 (act=relu, inact=relu, outact=none).  Anything else renders in the
 * compiler-scheduled modes (R2L_PREC_FP16X3, _FP16X1) only: the generated kernels are specialised, and r2l_set_precision /
 * r2l_load_weights refuse them with a message (`--precision auto` then stays in fp16x3). */
int r2l_set_activations(r2l_ctx* ctx, float head_slope, float inner_slope, float out_slope);
/* ... and the body architecture: block_residual = 1 is `--trial.body_arch resmlp` (x = outact(x + W2 inact(W1 x + b1) + b2),
 * model/nerf_raybased.py:461-465), 0 is `--trial.body_arch mlp` with an even number of body layers (:515-518: Linear + act repeated;
 * two consecutive layers ride in one "block": x = act(W2 act(W1 x + b1) + b2), the tensors passed as body.{i}.body.{0,2}.*).
 * r2l_set_activations(...) = r2l_set_network_form(..., 1). */
int r2l_set_network_form(r2l_ctx* ctx, float head_slope, float inner_slope, float out_slope, int block_residual);
/* Override PointSampler.z_vals (model/nerf_raybased.py:88-90).  r2l_create fills them with
 * near*(1-t)+far*t, t = linspace(0,1,n) by the scalar formula; torch.linspace on the CPU is
 * vector-width dependent in the last ulp (AVX2 vs AVX-512 builds differ), so a front-end
 * that wants bit-identical points to the reference running on the same host passes the
 * tensor the reference would have computed.  z_host: n_sample floats on the host. */
int r2l_set_z_vals(r2l_ctx* ctx, const float* z_host, int n);

/* Render rows [row_begin,row_end) of n_pose frames.  c2w: n_pose x [3,4] row-major f32
 * (the reference's c2w[:3,:4]), on the host if c2w_on_device == 0 (n_pose must be 1) or
 * in device memory otherwise.  rgb_out_dev: [n_pose, (row_end-row_begin)*W, 3] f32. */
int r2l_render(r2l_ctx* ctx, const float* c2w, int c2w_on_device, int n_pose,
               int row_begin, int row_end, float* rgb_out_dev, void* stream);

/* Given-rays variant: rays_o_dev, rays_d_dev [n,3] f32 device; rgb_out_dev [n,3]. */
int r2l_render_rays(r2l_ctx* ctx, const float* rays_o_dev, const float* rays_d_dev, int n,
                    float* rgb_out_dev, void* stream);

/* Stand-alone K1+K2 (parity / API mirror of PointSampler.sample_test and
 * PositionalEmbedder.__call__): either output may be NULL.
 * pts_out_dev [rows*W, 48], emb_out_dev [rows*W, 1008]; c2w on the host. */
int r2l_sample_embed(r2l_ctx* ctx, const float* c2w_host, int row_begin, int row_end,
                     float* pts_out_dev, float* emb_out_dev, void* stream);
/* PositionalEmbedder on caller-provided points: x_dev [n, dim] -> emb_out_dev [n, dim*21] */
int r2l_embed(const float* x_dev, int n, int dim, int L, float* emb_out_dev, void* stream);

/* Host-only (no GPU): pack state_dict tensors into the MFMA chunk stream that
 * r2l_load_weights uploads (csrc/r2l_common.h); for the CPU tests of the host logic.
 * Returns the image size in bytes (negative on error), copies at most cap bytes to out. */
long long r2l_debug_pack_host(const float* const* tensors, int n_tensors, int n_block,
                              int precision_mode, char* out, long long cap);

/* Host-only: the R2L_PREC_FP16_FP8 body stream (28 KiB chunks | 4 KiB aux blocks | tail weights) that
 * r2l_load_weights uploads for r2l_body_kernel; offs[0] / offs[1] receive the aux / tail byte offsets. */
long long r2l_debug_pack_body_host(const float* const* tensors, int n_tensors, int n_block,
                                   char* out, long long cap, long long* offs);
/* which stream the call above packs (thread-local): 0 = R2L_PREC_FP16_FP8's (bf6 terms, 28 KiB chunks; the default),
 * 1 = R2L_PREC_FP16_E4M3's (32 KiB chunks), 2 = the 'bf6r' experiment (bf6 terms, the bf6(W) operands converted on chip from
 * the fp16 fragments: 22 KiB chunks; csrc/r2l_common.h R2L_BF6R_STREAM) */
int r2l_debug_pack_body_format(int fmt);
/* The hand-scheduled body kernel alone (R2L_PREC_FP16_FP8): x_out = ResMLP blocks(x_in) on n_tiles ray
 * tiles in the register-image layout [tile][wave 4][group 32][lane 64][4] f32: group 4u + g of lane 32h + ray holds
 * features 32u + 8g + 4h .. + 3 (csrc/r2l_common.h); parity tests only. */
int r2l_debug_body(r2l_ctx* ctx, const float* x_in_dev, float* x_out_dev, int n_tiles, void* stream);
/* R2L_PREC_FP16_FP8, networks with the global skip: the body kernel ends every ray tile with the tail layer
 * (rgb = sigmoid(W_t (x + h) + b_t), model/nerf_raybased.py:539-544) straight from its registers.  on = 0 selects the
 * three-launch form (body kernel writes x, r2l_tail_kernel finishes) that networks without the skip always use;
 * parity tests compare the two. */
int r2l_debug_set_fused_tail(r2l_ctx* ctx, int on);

/* R2L_PREC_FP16_FP8 converts every operand set of the ResMLP body (the input x of block b, its hidden h) to bf6 with
 * ONE power-of-two scale per set: activations (x act_scale = 16) / 2^E must fit bf6's +-28.  The 2 n_block + 1 exponents
 * E (x_0, h_0, x_1, h_1, ..., x_n_block) are measured by the library itself: the first R2L_PREC_FP16_FP8 render after
 * r2l_load_weights evaluates the body in fp32 on a sample of that call's own rays (up to 1,024, behind its head launch)
 * and writes the exponents into the weight stream before its body launch -- device work in stream order, no host
 * round trip; other streams must not render with the context until that call has been enqueued.  A call of fewer than
 * 1,024 rays is a thin sample: its maxima are used and kept, and the following calls add theirs (exponents only grow)
 * until one call has filled the sample.  Ranks that render row shards of the same frames see different rays: exchange
 * the exponents once (r2l_get_act_exponents, element-wise maximum over the ranks, r2l_set_act_exponents; the Python
 * side does it in dist.agree_act_exponents) so that every shard is rendered with the same arithmetic.
 * r2l_set_act_exponents fixes them instead (NULL: measure again on the next render; synchronous host copy),
 * r2l_get_act_exponents reads back what the kernel uses (synchronous). */
int r2l_set_act_exponents(r2l_ctx* ctx, const int* exps, int n);
int r2l_get_act_exponents(r2l_ctx* ctx, int* out, int n);

/* Range tracking of R2L_PREC_FP16_FP8 (the reference has no counterpart: its fp32 path has no operand ranges,
 * model/nerf_raybased.py:443-465, 539-544).  The exponents above come from a sample of the first call's rays; whether
 * they hold for the rays rendered SINCE is measured, not assumed:
 *   - every head launch adds the largest h0 (= the body's first operand set) of EVERY ray it renders to a running
 *     maximum (cost: 64 VALU per 128-ray tile);
 *   - the first body launch after r2l_load_weights and every guard_period-th one afterwards (default 8; 1 = every
 *     launch, 0 = never) runs the range-guard build of the body kernel: bit-identical results, and per operand set
 *     (IN_b, H_b: 2 n_block) the maximum |a| over every ray of that launch (r2l_body_guard_kernel: 2 v_max3_f32 per 4
 *     values, +1.2 % kernel time when it runs, i.e. +0.15 % at the default period).
 * r2l_get_range_status reads the words (synchronises the stream of the newest render) and relates them to the exponents
 * in use: fill = max * 16 / 2^E / 28 is the fraction of bf6's +-28 the largest value of a set reached; the calibration
 * aims at <= 16/28 = 0.571, values beyond 1 were clamped.  reset != 0 clears the words and the launch counters.
 * Cost: one stream synchronisation and ONE device-to-host copy (range word, the 2 n_block maxima and the 2 n_block + 1
 * exponents live in one allocation); r2l_get_act_exponents likewise one copy, r2l_set_act_exponents one copy + one launch.
 * Under HIP-graph capture the choice "range-guarded or not" is host state evaluated when the launch is ENQUEUED: a
 * captured graph replays the build it captured (every replay guarded, or none), and the launch counters of
 * r2l_range_status count enqueues, not replays (the maxima themselves are device words and do keep accumulating when the
 * captured build is the guarded one).  Capture with guard_period 0 and run one eager range-guarded render every so many
 * replays, or capture the guarded build (+1.2 %).
 * r2l_recalibrate (stream-ordered device work) replaces the exponents by those the collected maxima ask for: what the
 * first call would have measured had it seen every ray of the guarded launches; frames rendered before it with
 * saturated sets should be rendered again. */
typedef struct r2l_range_status {
    float h0_max;            /* largest head output (real units) over every ray since the last reset */
    float h0_fill;           /* its fill of operand set 0 under the exponents in use */
    float worst_fill;        /* largest fill over the 2 n_block operand sets of the guarded launches since the reset */
    int worst_set;           /* its set index (2b: input of block b, 2b+1: hidden layer of block b), -1: no guarded launch */
    int saturated;           /* a fill reached 1: values were clamped to +-28 */
    int beyond_calibration;  /* a fill exceeds 16 / format_top: r2l_recalibrate would raise that set's exponent */
    float format_top;        /* largest magnitude of the operand format in use: 28 (bf6), 448 (e4m3) */
    float stream_max;        /* largest |activation| (real units) of any operand set seen since the reset: the error of the
                              * low-precision terms is proportional to it (`--precision auto` decides on it) */
    long long launches;          /* R2L_PREC_FP16_FP8 body launches since the last reset */
    long long guarded_launches;  /* ... of them range-guarded */
} r2l_range_status;
int r2l_set_guard_period(r2l_ctx* ctx, int period);
int r2l_get_range_status(r2l_ctx* ctx, r2l_range_status* out, int reset);
int r2l_recalibrate(r2l_ctx* ctx, void* stream);

/* introspection for bench.py / DESIGN.md */
long long r2l_flops_per_ray(const r2l_ctx* ctx);      /* algorithmic: 2*MACs of the network */
/* algorithmic flops per ray of the kernel the timing events bracket: the whole network for the single-kernel
 * modes, the 2*n_block body layers (r2l_body_kernel) for R2L_PREC_FP16_FP8 */
long long r2l_kernel_flops_per_ray(const r2l_ctx* ctx);
long long r2l_weight_image_bytes(const r2l_ctx* ctx); /* packed fp16 image streamed per ray tile */
int r2l_rays_per_tile(const r2l_ctx* ctx);
/* HIP-event timing of the dominant kernel on the stream it is launched on: when enabled,
 * every r2l_render* call records start/stop events around its kernel; r2l_kernel_time_ms
 * synchronises those events and returns the sum and count since the last reset. */
int r2l_timing_enable(r2l_ctx* ctx, int on);
int r2l_kernel_time_ms(r2l_ctx* ctx, double* total_ms, int* n_launches, int reset);

/* ---------------------------------------------------------------------------------
 * NeRF teacher (coarse 64 + fine 128 samples).  Replaces:
 *   render(H,W,focal,chunk,c2w=...)   main.py:107-186 (c2w path) / create_data.py:824
 *   render_rays                       main.py:624-756
 *   run_network + Embedder + NeRF     main.py:65-87, helpers:24-56, model/nerf_raybased.py:377-401
 *   raw2outputs                       main.py:556-621
 *   sample_pdf                        utils/run_nerf_raybased_helpers.py:283-330
 *   sort(cat(z_vals, z_samples))      main.py:730-732
 * --------------------------------------------------------------------------------- */
int nerf_create(nerf_ctx** out, int H, int W, double focal, float near_, float far_,
                int N_samples, int N_importance, int multires, int multires_views,
                int white_bkgd, int precision_mode);
void nerf_destroy(nerf_ctx* ctx);
/* which: 0 = network_fn (coarse), 1 = network_fine.  tensors: 24 HOST pointers in
 * state_dict order: pts_linears.{0..7}.{weight,bias}, views_linears.0.{weight,bias},
 * feature_linear.{weight,bias}, alpha_linear.{weight,bias}, rgb_linear.{weight,bias}.
 * A load that is refused leaves THAT network unloaded (the other one is not touched): renders return R2L_ESTATE until it is
 * loaded again. */
int nerf_load_weights(nerf_ctx* ctx, int which, const float* const* tensors, int n_tensors);
int nerf_set_precision(nerf_ctx* ctx, int precision_mode);
/* one mode per network: coarse_mode for network_fn's launches, fine_mode for network_fine's (main.py:700-741).  The fine samples
 * are drawn from the coarse pass's weights (sample_pdf, helpers:283-330): on rays that graze an object those weights are ~0 and
 * the pdf is decided by differences at the 1e-4 level, so a trained teacher needs the coarse pass at fp32 grade (FP16X3) whatever
 * the fine pass runs in (profiles/r05_trained_like.txt).  All or nothing: when either network's image for its new mode
 * cannot be built, both networks keep the modes they had. */
int nerf_set_precision_pair(nerf_ctx* ctx, int coarse_mode, int fine_mode);
/* on != 0: for callers that drop render()'s extras, as the reference's own do (main.py:277-282, utils/create_data.py:824-831) -- the render
 * pipeline (nerf_render / nerf_render_rays[_ex]) leaves out work whose results only the extras rgb0 / raw would show:
 *   - the COARSE network runs without its view branch (feature_linear, views_linears.0, rgb_linear: model/nerf_raybased.py:391-398) whenever
 *     its mode is R2L_PREC_FP16X3_ASM: sample_pdf and every map of the fine pass depend on it through its densities only (main.py:716-733),
 *     which are computed bit for bit as before; rgb0 (main.py:743) is NOT computed and nerf_copy_extras refuses to return it;
 *   - the FINE network (mode R2L_PREC_FP16X3_ASM or R2L_PREC_FP16_MIX, no density noise) computes the alpha row first and skips the feature
 *     rows, the views layer and the rgb layer for workgroup tiles (128 consecutive points) none of whose densities is positive: alpha = 0,
 *     weight 0 exactly (main.py:600-606), so their colours cannot reach rgb_map; `raw` shows zeros for them.
 * rgb / disp / acc / depth, disp0 / acc0 / z_samples / z_std are bit for bit what they are without the flag.  nerf_run_network always evaluates
 * the whole network.  Default: off. */
int nerf_set_skip_rgb0(nerf_ctx* ctx, int on);
/* Override the coarse depths z_vals[N_samples] (main.py:676-678) and/or the inverse-CDF
 * abscissae u[N_importance] = torch.linspace(0,1,N) (helpers:293) with the tensors the
 * reference computes on this host (torch.linspace's last ulp is CPU-vector-width dependent;
 * nerf_create fills both with the scalar formula).  Either pointer may be NULL. */
int nerf_set_sampling(nerf_ctx* ctx, const float* z_coarse_host, int n_z, const float* u_host, int n_u);
/* rows [row_begin,row_end) of one frame; c2w [3,4] on host.  Outputs are device
 * pointers, any of disp/acc/depth may be NULL.  rgb [n,3], others [n]. */
int nerf_render(nerf_ctx* ctx, const float* c2w_host, int row_begin, int row_end,
                float* rgb_dev, float* disp_dev, float* acc_dev, float* depth_dev, void* stream);
int nerf_render_rays(nerf_ctx* ctx, const float* rays_o_dev, const float* rays_d_dev, int n,
                     float* rgb_dev, float* disp_dev, float* acc_dev, float* depth_dev,
                     void* stream);
/* coarse-pass by-products of the last nerf_render* call (device pointers owned by ctx,
 * valid until the next call): rgb0 [n,3], z_samples [n,N_importance], z_vals [n,S0+S1] */
int nerf_last_extras(nerf_ctx* ctx, const float** rgb0, const float** z_samples,
                     const float** z_vals, const float** raw_fine);
/* stream-ordered device-to-device copies of those by-products for the first n rays of the
 * last call into caller tensors (any may be NULL): rgb0 [n,3], z_samples [n,N_importance],
 * z_vals [n,S0+S1], raw_fine [n,S0+S1,4] */
int nerf_copy_extras(nerf_ctx* ctx, int n, float* rgb0_dev, float* z_samples_dev, float* z_vals_dev,
                     float* raw_dev, void* stream);
/* disp0 [n], acc0 [n] of the coarse pass and z_std [n] = std(z_samples, unbiased=False): the rest of
 * render_rays' return set (main.py:743-750); any pointer may be NULL */
int nerf_copy_extras0(nerf_ctx* ctx, int n, float* disp0_dev, float* acc0_dev, float* z_std_dev, void* stream);
/* render_rays with the training-time randomness of the reference supplied by the caller (each pointer may be
 * NULL = the deterministic test path): z_coarse_dev [n,N_samples] jittered coarse depths (perturb > 0,
 * main.py:684-699), u_dev [n,N_importance] (sample_pdf det=False, helpers:298-307), noise0_dev [n,N_samples] /
 * noise1_dev [n,N_samples+N_importance] = randn * raw_noise_std (main.py:592-600) */
int nerf_render_rays_ex(nerf_ctx* ctx, const float* rays_o_dev, const float* rays_d_dev, int n,
                        const float* z_coarse_dev, const float* u_dev, const float* noise0_dev,
                        const float* noise1_dev, float* rgb_dev, float* disp_dev, float* acc_dev,
                        float* depth_dev, void* stream);

/* HIP-event timing of the teacher's MLP launches (nerf_chain_kernel / nerf_mlp_kernel: 99 % of a frame) on the stream they
 * are launched on, as r2l_timing_enable / r2l_kernel_time_ms: sum and count since the last reset (bench.py's create_data
 * and teacher legs). */
/* parity tests / A-B timing: 1 = the coarse pass's raw2outputs, sample_pdf and merge as three launches instead of the one fused
 * launch of the deterministic path (nerf_coarse_scan_kernel); the results are bit-identical */
int nerf_debug_set_split_scans(nerf_ctx* ctx, int on);
/* A-B timing / parity tests: 16-point column tiles per wave of this context's FP16X1 chain, 4 (default: 256-point workgroup
 * tiles), 3 (192) or 2 (128); the results are bit-identical (the arithmetic per point does not depend on the tiling) */
int nerf_debug_set_x1_col_tiles(nerf_ctx* ctx, int n);
/* A-B timing / parity tests: 0 = the four-tile FP16X1 chain with its embedding computed by HIP code between two tile blocks
 * (nerf_chain_kernel<true, 4>, round 4) instead of inside the generated stream (nerf_chain_emb_kernel, round 5); bit-identical */
int nerf_debug_set_x1_stream_embed(nerf_ctx* ctx, int on);
int nerf_timing_enable(nerf_ctx* ctx, int on);
int nerf_kernel_time_ms(nerf_ctx* ctx, double* total_ms, int* n_launches, int reset);

/* Host-only (no device call): the shuffle of `create_data rand` -- utils/create_data.py:858-859 draws two
 * np.random.permutation(n) per save group from the one global numpy stream (create_data.py:18), n = 16,000,000 rays at
 * the reference's sizes; every rank has to walk that stream, so it is the serial piece of config 5.  numpy's legacy
 * RandomState.permutation restated (arange + Fisher-Yates with random_interval's masked rejection on MT19937 words):
 * mt_key624 / mt_pos are the state of RandomState.get_state() and are advanced in place (set_state them back), out[n]
 * receives the permutation as 32-bit indices.  Bit-identical to numpy, 5-20x faster (csrc/np_shuffle.hip). */
int r2l_np_legacy_permutation(unsigned* mt_key624, int* mt_pos, long long n, int* out);

/* Forward-facing scenes (render(..., ndc=True), main.py:148-162): when on, nerf_render and
 * nerf_render_rays take the view directions from the given (world-space) rays, project the rays
 * with ndc_rays(H, W, focal, ndc_near, ...) and sample / composite along the projected rays; the
 * context's near / far are then NDC depths (0 and 1 in the reference, main.py:917-918). */
int nerf_set_ndc(nerf_ctx* ctx, int on, float ndc_near);
/* ndc_rays (utils/run_nerf_raybased_helpers.py:260-279): n rays [n,3] -> projected [n,3] pairs. */
int nerf_ndc_rays(int H, int W, double focal, float near_, const float* rays_o_dev,
                  const float* rays_d_dev, int n, float* out_o_dev, float* out_d_dev, void* stream);

/* get_rays (utils/run_nerf_raybased_helpers.py:231-257) for rows [row_begin,row_end):
 * rays_o_dev, rays_d_dev [rows*W, 3]; c2w [3,4] on the host. */
int nerf_get_rays(int H, int W, double focal, const float* c2w_host, int row_begin, int row_end,
                  float* rays_o_dev, float* rays_d_dev, void* stream);
/* run_network (main.py:65-87): points o + d*z for z_dev [n,S] (z_stride = S) or one shared
 * row (z_stride = 0), both embedders, network `which` -> raw_dev [n,S,4] = (rgb, sigma). */
int nerf_run_network(nerf_ctx* ctx, int which, const float* rays_o_dev, const float* rays_d_dev,
                     const float* z_dev, int z_stride, int S, int n, float* raw_dev, void* stream);
/* the same with GIVEN view directions viewdirs_dev [n,3], one per ray, embedded as they are (main.py:76-77) instead of
 * rays_d / |rays_d|: what a forward-facing render hands its networks (view directions of the world rays, points along the
 * projected rays: main.py:148-162).  viewdirs_dev = NULL is exactly nerf_run_network. */
int nerf_run_network_dirs(nerf_ctx* ctx, int which, const float* rays_o_dev, const float* rays_d_dev,
                          const float* viewdirs_dev, const float* z_dev, int z_stride, int S, int n,
                          float* raw_dev, void* stream);

/* Host-only: the R2L_PREC_FP16_FP8 image of one teacher network that nerf_load_weights uploads for
 * nerf_chain_kernel (the layer chain's weight stream followed by the 16 KiB bias / scale table; layout:
 * csrc/nerf_capi.hip pack_chain, restated by csrc/gen/nerf_gen.py pack_teacher).  tensors: the 24 state_dict
 * tensors (model/nerf_raybased.py:357-375).  Returns the image size in bytes (negative on error), copies at
 * most cap bytes to out; offs[0] receives the byte offset of the table. */
/* fmt: which stream -- 0 = fp16 + bf6 terms (R2L_PREC_FP16_FP8), 1 = fp16 only (R2L_PREC_FP16X1), 2 = hi | lo fragments of W x 2^k
 * (R2L_PREC_FP16X3_ASM) */
long long nerf_debug_pack_chain_host(const float* const* tensors, int n_tensors, int fmt, char* out, long long cap,
                                     long long* offs);

/* stand-alone scan kernels (all device pointers, f32):
 * raw [n,S,4], z [n,S], rays_d [n,3] -> rgb [n,3], disp [n], acc [n], weights [n,S], depth [n]
 * (weights/depth/disp/acc may be NULL). */
int nerf_raw2outputs(const float* raw, const float* z, const float* rays_d, int n, int S,
                     int white_bkgd, float* rgb, float* disp, float* acc, float* weights,
                     float* depth, void* stream);
/* the same with noise_dev [n,S] (or NULL) added to the density before the relu: raw_noise_std > 0,
 * main.py:592-600; the caller draws randn * raw_noise_std (or the pytest numpy stream) as the reference does */
int nerf_raw2outputs_noise(const float* raw, const float* z, const float* rays_d, const float* noise_dev,
                           int n, int S, int white_bkgd, float* rgb, float* disp, float* acc,
                           float* weights, float* depth, void* stream);
/* bins [n,n_bins], weights [n,n_bins-1] -> samples [n,N] (det=True: u = linspace(0,1,N), evaluated
 * in the kernel by the scalar formula).  The float sums follow ATen's CPU orders (the reference runs
 * sample_pdf on the CPU, main.py:723-728): torch.sum = 8-lane x 4-accumulator cascade, cumsum = double
 * accumulation rounded per element.  All three entry points are stream-ordered and allocate nothing. */
int nerf_sample_pdf(const float* bins, const float* weights, int n, int n_bins, int N,
                    float* samples, void* stream);
/* same with caller-provided u_dev [N] (device) */
int nerf_sample_pdf_u(const float* bins, const float* weights, int n, int n_bins,
                      const float* u_dev, int N, float* samples, void* stream);
/* general form: u_dev NULL (linspace), [N] (u_per_ray = 0) or [n,N] (u_per_ray = 1: det = False, the
 * caller draws u as helpers:298-307 does); optional parity taps cdf_out_dev [n,n_bins] (= cat(0, cumsum(pdf)))
 * and inds_out_dev [n,N] int32 (= searchsorted(cdf, u, right=True)) */
int nerf_sample_pdf_ex(const float* bins, const float* weights, int n, int n_bins, const float* u_dev,
                       int u_per_ray, int N, float* samples, float* cdf_out_dev, int* inds_out_dev,
                       void* stream);
/* a [n,na] and b [n,nb], each row ascending -> out [n,na+nb] ascending, = torch.sort(cat(a, b), stable): every NaN behind every
 * number (a row's NaNs trail it), a's element first on a tie; every slot of out is written */
int nerf_merge_sorted(const float* a, int na, const float* b, int nb, int n, float* out,
                      void* stream);
/* x [n,N] -> out [n,N], every row ascending as torch.sort orders floats (-inf ... +inf, then the NaNs); N <= 256 */
int nerf_sort_rows(const float* x, int n, int N, float* out, void* stream);

/* ---- generic fp32 layer path (csrc/r2l_generic.hip) ---------------------------------------------------------------
 * The variants the reference's constructors accept that the fused kernels are not built for: NeRF_v3_2 with netwidth != 256,
 * --layerwise_netwidths, trial.n_learnable != 2, n_sample_per_ray != 16, multires != 10, odd mlp depths
 * (model/nerf_raybased.py:483-537); NeRF with netdepth / netwidth other than 8 x 256 (:339-401).  One launch per nn.Linear,
 * fp32 products and accumulation on the fp32 MFMA (the reference's own precision), activations through HBM in caller buffers.
 * The host mirror composes them (efficient-nerf_amd/generic.py). */
typedef struct r2l_linear r2l_linear;
#define R2L_ACT_NONE 0
#define R2L_ACT_RELU 1      /* nn.ReLU */
#define R2L_ACT_LRELU 2     /* nn.LeakyReLU(), slope 0.01 (model/nerf_raybased.py:468-476) */
#define R2L_ACT_SIGMOID 3   /* the tail's nn.Sigmoid (:534-537) */
/* one nn.Linear: w_host [out_dim, in_dim] row-major as in the state_dict, b_host [out_dim] or NULL; copied to the device */
int r2l_linear_create(r2l_linear** out, const float* w_host, const float* b_host, int out_dim, int in_dim);
void r2l_linear_destroy(r2l_linear* lin);
/* y[r, :out] = post[r, :] + act((x[r, :in] W^T + b) * res_scale + res[r, :])  for r < n; res_dev / post_dev may be NULL (then
 * res_scale is not applied); row strides ld* in floats (>= the row's width: a layer can read a column slice of a wider buffer
 * and write into one, which is how the reference's torch.cat inputs are formed).  res_dev / post_dev may alias y_dev; x_dev
 * must not overlap y_dev.  ResMLP.forward (model/nerf_raybased.py:461-465): res = the block's input, act = outact;
 * NeRF_v3_2.forward's global skip (:542): post = the head's output on the last body layer. */
int r2l_linear_forward(const r2l_linear* lin, const float* x_dev, long long ldx, int n, float* y_dev, long long ldy,
                       const float* res_dev, long long ldr, float res_scale, int act, const float* post_dev, long long ldp,
                       void* stream);
/* PointSampler.sample_test / sample_train (model/nerf_raybased.py:100-102, 114-126) for any n_sample, and main.py:701 with
 * per-ray z: pts[r, 3 s + k] = rays_o[r, k] + rays_d[r, k] * z[s] (z_per_ray = 0: z_dev [n_sample]; 1: z_dev [n, n_sample]) */
int r2l_sample_points(const float* rays_o_dev, const float* rays_d_dev, int n, const float* z_dev, int n_sample, int z_per_ray,
                      float* pts_out_dev, void* stream);
/* Embedder.embed (utils/run_nerf_raybased_helpers.py:24-56; include_input, log_sampling): out[r, :] = [x, sin(x), cos(x),
 * sin(2 x), cos(2 x), ..., cos(2^(multires-1) x)] of x = x_dev[r, :dim]; row strides ldi / ldo in floats */
int nerf_embed(const float* x_dev, long long ldi, int n, int dim, int multires, float* out_dev, long long ldo, void* stream);

/* ---- training of the R2L student (csrc/r2l_train.hip; host mirror: efficient-nerf_amd/train.py) ----
 * Exact fp32 on the fp32 MFMA, one launch per layer and direction, every buffer the caller's.  Nothing here uses float atomics:
 * the same inputs give the same bits.  With n = 0 the per-ray buffers may be NULL (an empty batch: g_W and g_b become zero). */
/* r2l_linear_forward on weights that live in caller device buffers (w_dev [out_dim, in_dim], b_dev [out_dim]) */
int r2l_linear_forward_dev(const float* w_dev, const float* b_dev, int out_dim, int in_dim, const float* x_dev, long long ldx, int n,
                           float* y_dev, long long ldy, const float* res_dev, long long ldr, float res_scale, int act,
                           const float* post_dev, long long ldp, void* stream);
/* The element-wise part of a layer's backward pass.  The layer computed y = post + act(u), u = scale * lin + res.  Given g_y:
 *   g_post = g_y (+ g_post when post_accumulate);  g_u = g_y * act'(y - post);  g_res = g_u (+ g_res when res_accumulate);
 *   g_z = scale * g_u.
 * post_dev / g_res_dev / g_post_dev may be NULL.  g_res_dev may be g_y_dev (in place), and g_post_dev may be g_res_dev (it then
 * receives g_y + g_u).  act' from the saved output: relu a > 0, lrelu a > 0 ? 1 : 0.01, none 1, sigmoid a (1 - a). */
int r2l_train_act_backward(const float* g_y_dev, long long ldg, const float* y_dev, long long ldy, const float* post_dev,
                           long long ldp, int n, int width, int act, float scale, float* g_z_dev, long long ldz, float* g_res_dev,
                           long long ldr, int res_accumulate, float* g_post_dev, long long ldq, int post_accumulate, void* stream);
/* g_x [n, in_dim] = g_z [n, out_dim] W [out_dim, in_dim] (+ g_x when accumulate: gradients that meet on one stream add up) */
int r2l_train_grad_input(const float* g_z_dev, long long ldz, int n, const float* w_dev, int out_dim, int in_dim, float* g_x_dev,
                         long long ldgx, int accumulate, void* stream);
/* g_W [out_dim, in_dim] = g_z^T x and g_b [out_dim] = the column sums of g_z (g_b_dev may be NULL), overwritten.  The rays are cut
 * into r2l_train_grad_weight_slabs of n slabs -- a function of n alone -- whose partial results go to workspace_dev (slabs *
 * (out_dim * in_dim + out_dim) floats) and are added in slab order by a second kernel. */
int r2l_train_grad_weight_slabs(int n);
int r2l_train_grad_weight(const float* g_z_dev, long long ldz, const float* x_dev, long long ldx, int n, int out_dim, int in_dim,
                          float* g_w_dev, float* g_b_dev, float* workspace_dev, long long workspace_floats, void* stream);
/* loss_dev[0] = mean over n x 3 of (rgb - target)^2; g_out_dev [n, 3] = 2 (rgb - target) / (3 n), times rgb (1 - rgb) when
 * through_sigmoid (the tail layer's g_z directly); err_dev [n] (may be NULL) = the mean over the channels of (rgb - target)^2.
 * workspace_dev: ceil(n / 256) floats. */
int r2l_train_mse_loss(const float* rgb_dev, const float* target_dev, int n, int through_sigmoid, float* g_out_dev, float* err_dev,
                       float* loss_dev, float* workspace_dev, long long workspace_floats, void* stream);
/* torch.optim.Adam's update with betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad over `count` parameters in flat
 * buffers; step = the 1-based count of updates including this one */
int r2l_train_adam(float* param_dev, const float* grad_dev, float* exp_avg_dev, float* exp_avg_sq_dev, long long count, double lr,
                   long long step, void* stream);
/* PointSampler.sample_train with perturb > 0 (model/nerf_raybased.py:117-123): z_out [n, n_sample] = lower + (upper - lower) *
 * t_rand over the strata of z_vals_dev [n_sample]; feeds r2l_sample_points with z_per_ray = 1 */
int r2l_train_jitter_z(const float* z_vals_dev, const float* t_rand_dev, int n, int n_sample, float* z_out_dev, void* stream);
/* The ordered sum of the ranks' gradients of a ray-sharded step: out_dev[i] = (...((w0 p0[i]) + w1 p1[i]) + ...) + w_{P-1} p_{P-1}[i]
 * for i < count, part k at parts_dev + k * pitch_floats.  Every product and every sum is rounded to fp32 on its own (no fused
 * multiply-add) in part order: the bits of torch's separate mul and add, whatever the launch shape.  weights: n_part floats on the
 * HOST, passed to the kernel by value; 1 <= n_part <= 64.  out_dev may be part 0 itself (no other overlap); count >= 0. */
int r2l_train_sum_parts(const float* parts_dev, long long pitch_floats, int n_part, const float* weights, long long count,
                        float* out_dev, void* stream);

/* ---- real images to ray rows (csrc/r2l_convert.hip; host mirror: efficient-nerf_amd/convert_data.py) ----
 * utils/convert_original_data_to_rays_blender.py:142-223 as one gather: out_dev [rows, 9] = (rays_o, rays_d, rgb) of the pixels
 * order_dev [rows] names (int64, device): order[k] = image * H * W + row * W + column on the output grid, H x W = H0 x W0, or
 * H0/2 x W0/2 with half_res.  images_dev: uint8 [n_img, H0, W0, channels], channels 3 or 4; poses_dev: float32 [n_img, 3, 4];
 * focal: of the output grid (already halved with half_res).  Colours are bytes / 255, under half_res the mean of the 2 x 2 block
 * (cv2.INTER_AREA for a factor of two); four channels are composited on white (rgb * a + (1 - a)), three are kept as they are.
 * Rays are get_rays' (:69-86).  One thread per row, plain stores, no atomics: the same inputs give the same bits.  An index outside
 * [0, n_img * H * W) reads nothing and leaves a row of NaN. */
int r2l_rays_from_images(const unsigned char* images_dev, int n_img, int H0, int W0, int channels, const float* poses_dev, double focal,
                         int half_res, const long long* order_dev, long long rows, float* out_dev, void* stream);

/* ---- rays for online distillation (csrc/r2l_online.hip; host mirror: efficient-nerf_amd/online.py) ----
 * n random rays of n_pose cameras: ray k belongs to pose k % n_pose and to the pixel mulhi32(x, H * W) of its H x W grid, x = word 0
 * of Philox4x32-10 with counter (k_lo, k_hi, step_lo, step_hi) and key (seed_lo, seed_hi); the relative bias of a pixel's share is
 * at most H * W / 2^32, and 1 <= H * W < 2^31.  poses_dev: float32 [n_pose, 3, 4]; focal_dev: float32 [n_pose], each pose's own focal.
 * rays_o_dev / rays_d_dev [n, 3] are get_rays' (utils/run_nerf_raybased_helpers.py:231-257) for that pixel, bit for bit what
 * nerf_get_rays writes for it; pixel_dev [n] (int64, may be NULL) receives row * W + column.  One thread per ray, plain stores, no
 * atomics: the output is a function of the arguments alone.  n = 0 is a no-op. */
int r2l_rand_rays(const float* poses_dev, const float* focal_dev, int n_pose, int H, int W, unsigned long long seed, long long step,
                  long long n, float* rays_o_dev, float* rays_d_dev, long long* pixel_dev, void* stream);

/* The random poses of an LLFF step, built on the device (host mirror: llff.pose_in_boxes, the reference's get_rand_pose_v2,
 * dataset/load_llff.py:187-236, with its draws given).  u_dev: float64 [n_pose, n_u] uniform draws in [0, 1), n_u = 7 or 6: the
 * position in its box (x, y, z), the viewing axis in its box (x, y, z) and, with n_u = 7, the focal scale u + 1 drawn after each
 * pose.  box_host: 27 doubles in HOST memory, passed to the kernel by value (llff.pose_box): the average pose c2w[:3, :4] row-major
 * (12), up (3), the widened position box left [3], right [3], the widened viewing-axis box left [3], right [3].  Pose k:
 * p = u (right - left) + left per axis; position and viewing axis are c2w . (p, 1), the translation added to both; the axis is
 * normalised, then view_matrix(axis, up, position).  poses_dev [n_pose, 3, 4] and focal_dev [n_pose] = focal (u6 + 1), or focal
 * with n_u = 6, are float32, ready for r2l_rand_rays.  Computed in binary64, one rounding per operation, each entry rounded to
 * float32 once; one thread per pose, plain stores, no atomics: the output is a function of the arguments alone.  A zero-length
 * vector gives NaN rows.  R2L_EINVAL: a NULL pointer, n_pose < 1, another n_u, a misaligned pointer, a focal that is not finite and
 * positive, a box entry that is not finite, a box with right <= left. */
int r2l_llff_rand_poses(const double* u_dev, int n_pose, int n_u, const double* box_host, double focal, float* poses_dev, float* focal_dev,
                        void* stream);

/* ---- FLIP of image pairs (csrc/r2l_flip.hip; host side: efficient-nerf_amd/metrics.py flip, flip_taps.py) ----
 * FLIP.compute_flip(a, b, pixels_per_degree) of utils/flip_loss.py:70-130, the TestFLIP of the reference's [TEST] lines, on
 * v = mul * (x - lo) + add of each image (three roundings, applied first; (0, 1, 0) is the identity, exactly): sRGB clamped to
 * [0, 1] -> linear RGB -> XYZ -> YCxCz, the three contrast-sensitivity filters with replicate padding, linear RGB clamped to the unit
 * box -> L*a*b* -> Hunt -> HyAB -> redistribution (q_c 0.7, p_c 0.4, p_t 0.95), edge and point detection on (Y + 16) / 116
 * (w 0.082, q_f 0.5, clamped to [0, 1]), result dE_c ^ (1 - dE_f).  Symmetric in its two images.  a_dev, b_dev: float32
 * [n_img, H, W, 3]; map_dev [n_img, H, W] or NULL; frame_mean_dev [n_img]: each frame's mean.  The filter radii follow from
 * pixels_per_degree as the reference derives them (10 and 9 at its default 67.02) and the taps are built on the host in float64;
 * every filter runs as two 1-D passes.  Radii up to 16 (pixels_per_degree <= 118.4), H and W up to 32768: R2L_EINVAL beyond.
 * workspace_dev: r2l_flip_workspace_floats(H, W, pixels_per_degree) floats (or a negative code), whatever n_img: the frames go
 * through it one after another.  Plain stores and fixed-order sums, no atomics: the same inputs give the same bits, and the means
 * are the same with and without a map.  n_img = 0 is a no-op. */
long long r2l_flip_workspace_floats(int H, int W, double pixels_per_degree);
int r2l_flip(const float* a_dev, const float* b_dev, int n_img, int H, int W, float a_lo, float a_mul, float a_add, float b_lo, float b_mul,
             float b_add, double pixels_per_degree, float* map_dev, float* frame_mean_dev, float* workspace_dev, long long workspace_floats,
             void* stream);
/* The 1-D taps r2l_flip filters with, for tests and tools (host only, no device): taps_host [7][33] float32, rows A, RG, BY1, BY2
 * (A = n (x) n, RG likewise, BY = t1 (x) t1 + t2 (x) t2; 2 radius_csf + 1 taps each, zeros behind) and G, D, P (edge = D (x) G,
 * point = P (x) G, first factor along x; 2 radius_feature + 1 taps). */
int r2l_flip_taps(double pixels_per_degree, float* taps_host, int* radius_csf, int* radius_feature);

/* ---- LPIPS of image pairs (csrc/r2l_lpips.hip; host side: efficient-nerf_amd/metrics.py LPIPS, load_lpips_weights) ----
 * LPIPS v0.1 with the AlexNet trunk (the reference's default --lpips_net alex), the TestLPIPS of its [TEST] lines, on
 * v = mul * (x - lo) + add of each image (three roundings, applied first; (0, 1, 0) is the identity, exactly; values are meant to lie
 * in [-1, 1]): the scaling layer (v - shift) / scale, torchvision's features 0 .. 11 (conv 3->64 11x11 stride 4 pad 2, ReLU,
 * max-pool 3x3 stride 2, conv 64->192 5x5 pad 2, ReLU, max-pool 3x3 stride 2, conv 192->384, 384->256, 256->256 3x3 pad 1, ReLU
 * each; zero padding, floor-mode pooling), and per ReLU output k the mean over the pixels of sum_c lin_k[c] (n_a[c] - n_b[c])^2 with
 * n = f / (sqrt(sum_c f_c^2) + 1e-10); d = sum_k d_k.  Symmetric in its two images; an identical pair gives 0.
 * r2l_lpips_create copies 15 host tensors to the current device once: the 5 conv weights [out, in, kh, kw] as the state_dict holds
 * them, the 5 biases, the 5 lin vectors [C_k] (C = 64, 192, 384, 256, 256), in this order.  a_dev, b_dev: float32 [n_img, H, W, 3];
 * d_dev [n_img]: each pair's d; layers_dev [n_img, 5]: each pair's d_k, or NULL.  H and W from 31 (the second pool needs 3 rows and
 * columns) to 32768: R2L_EINVAL beyond.  workspace_dev: r2l_lpips_workspace_floats(H, W) floats (or a negative code), whatever n_img:
 * the pairs go through it in groups whose size follows from H and W alone (8 pairs of frames up to about 400 x 400, 1 pair from about
 * 1100 x 1100).  The convolutions are a patch gather and the fp32 MFMA layer of r2l_linear_forward_dev;
 * plain stores and fixed-order sums, no atomics: the same inputs give the same bits, a pair's value does not depend on n_img or on
 * its place in the stack, and d is the same with and without layers_dev.  n_img = 0 is a no-op. */
typedef struct r2l_lpips_ctx r2l_lpips_ctx;      /* the function below has the plain name */
int r2l_lpips_create(r2l_lpips_ctx** out, const float* const* tensors_host, int n_tensors);
void r2l_lpips_destroy(r2l_lpips_ctx* l);
long long r2l_lpips_workspace_floats(int H, int W);
int r2l_lpips(const r2l_lpips_ctx* l, const float* a_dev, const float* b_dev, int n_img, int H, int W, float a_lo, float a_mul, float a_add, float b_lo,
              float b_mul, float b_add, float* d_dev, float* layers_dev, float* workspace_dev, long long workspace_floats, void* stream);

/* ---- Motion-JPEG frames (csrc/r2l_mjpeg.hip; host side: efficient-nerf_amd/video.py) ----
 * Each frame of rgb_dev, float32 [n_img, H, W, 3], becomes one complete baseline JPEG file (ITU-T T.81: sequential DCT, 8 bit, Huffman):
 * Y, Cb, Cr in the JFIF colour space, 4:4:4 (every sampling factor 1), one interleaved scan, no restart markers.  A pixel is
 * p = floor(255 clamp(x, 0, 1)), the front end's to8b, with NaN = 0; H and W are padded up to multiples of 8 by repeating the last row
 * and column; Y = 0.299 R + 0.587 G + 0.114 B - 128, Cb = -0.168736 R - 0.331264 G + 0.5 B, Cr = 0.5 R - 0.418688 G - 0.081312 B and the
 * FDCT of T.81 A.3.3 in fp32; coefficients are divided by the quantiser and rounded to nearest, AC clamped to +-1023.  The quantisers
 * are Annex K.1 / K.2 scaled by libjpeg's rule (s = 5000 / q below 50, else 200 - 2 q; entry = clamp((t s + 50) / 100, 1, 255)),
 * quality 1 .. 100; the Huffman tables are Annex K.3.3's.  Each component predicts its DC from the previous block in raster order,
 * from 0 at the start of every frame; frames do not depend on each other.
 * r2l_mjpeg_tables: the two quantisers in zig-zag order, as DQT stores them (host only).  r2l_mjpeg_header: the bytes in front of the
 * scan, SOI APP0 (JFIF 1.01) DQT DQT SOF0 DHT x 4 SOS, into out_host (room for cap bytes); returns their number, 623 (host only).
 * r2l_mjpeg_max_frame_bytes: a bound on header + byte-stuffed scan + EOI.  r2l_mjpeg_workspace_bytes: what r2l_mjpeg_encode needs for
 * n_img frames at once.  All three return a negative code on a bad argument.
 * r2l_mjpeg_encode: out_dev + k * out_pitch holds frame k's file (FF D8 ... FF D9), sizes_dev[k] (int64) its length; out_pitch at
 * least r2l_mjpeg_max_frame_bytes.  coef_dev, int16 [n_img, n_blocks, 3, 64] or NULL: the quantised coefficients in zig-zag order, the DC
 * before prediction, blocks in raster order.  Nothing is allocated or copied; the launches go to `stream`, the only atomic is an OR
 * into cleared words, so the same input gives the same bytes.  H and W from 1 to 65535, n_img up to 65535, rgb_dev 4-byte, sizes_dev 8-byte,
 * workspace_dev and coef_dev 16-byte aligned: R2L_EINVAL otherwise, before a device is touched.  n_img = 0 is a no-op. */
int r2l_mjpeg_tables(int quality, unsigned char* luma64, unsigned char* chroma64);
long long r2l_mjpeg_header(int H, int W, int quality, unsigned char* out_host, long long cap);
long long r2l_mjpeg_workspace_bytes(int n_img, int H, int W);
long long r2l_mjpeg_max_frame_bytes(int H, int W);
int r2l_mjpeg_encode(const float* rgb_dev, int n_img, int H, int W, int quality, void* workspace_dev, long long workspace_bytes,
                     unsigned char* out_dev, long long out_pitch, long long* sizes_dev, short* coef_dev, void* stream);

/* ---- PNG files (csrc/r2l_png.hip; host side: efficient-nerf_amd/png.py) ----
 * Each frame of rgb_dev, float32 [n_img, H, W, 3], becomes one complete PNG file: 8-bit RGB (colour type 2), non-interlaced, a byte
 * p = floor(255 clamp(x, 0, 1)) as in the JPEG frames above (NaN = 0).  filter: -1 gives every row the type (None, Sub, Up, Average,
 * Paeth) with the smallest sum of |residual as int8|, ties to the lowest type; 0 .. 4 forces that type on every row.  The filtered
 * stream, H rows of 1 + 3 W bytes, is cut into segments of whole rows that are compressed independently of each other: matches are
 * runs (distance 1, length 3 .. 258) that do not reach back over the segment's start, each segment is one deflate block with dynamic
 * Huffman codes (lengths limited to 15 bits, 7 for the code-length code) or, where that is no shorter, one stored block; every segment
 * but the last is closed with an empty stored block and is one IDAT chunk.  Adler-32 and every chunk's CRC-32 are computed on the device.
 * r2l_png_layout: the rows of a segment (as many as give at most 16 KiB of filtered bytes, at least one) and the segments of a frame.
 * r2l_png_max_frame_bytes: a bound on the file for any input (every segment stored).  r2l_png_workspace_bytes: what r2l_png_encode
 * needs for n_img frames at once.  The two sizes return a negative code on a bad argument (host only, all three).
 * r2l_png_encode: out_dev + k * pitch holds frame k's file, sizes_dev[k] (int64) its length; pitch at least r2l_png_max_frame_bytes.
 * Nothing is allocated or copied and the host does not wait; the launches go to `stream`; the atomics are integer adds in LDS and ORs
 * into cleared words, so the same input gives the same bytes, and a frame's file does not depend on the other frames.  H and W from 1 to
 * 16384, n_img up to 65535, rgb_dev 4-byte, sizes_dev 8-byte, workspace_dev 16-byte aligned: R2L_EINVAL otherwise, before a device is
 * touched.  n_img = 0 is a no-op. */
long long r2l_png_max_frame_bytes(int H, int W);
long long r2l_png_workspace_bytes(int n_img, int H, int W);
int r2l_png_layout(int H, int W, int* rows_per_segment, int* n_segments);
int r2l_png_encode(const float* rgb_dev, int n_img, int H, int W, int filter, void* workspace_dev, long long workspace_bytes,
                   unsigned char* out_dev, long long pitch, long long* sizes_dev, void* stream);

/* ---- PNG files read (csrc/png_inflate.h, csrc/r2l_png_decode.hip; host side: png.decode_pngs) ----
 * n_img zlib streams (the concatenated IDAT payloads of 8-bit, non-interlaced files of one shape, C = 1, 2, 3 or 4 bytes per pixel) become
 * pixels: stream k is zstreams_dev[offsets_dev[k] .. offsets_dev[k + 1]), its picture out_dev[k] of uint8 [n_img, H, W, C].  One
 * workgroup of one wave per stream inflates it (stored, fixed and dynamic blocks, the Adler-32 verified) into the workspace through a
 * 64 KiB window in LDS; a second launch undoes the five row filters, 64 rows at a time on a skewed wavefront.  Every read of a stream is
 * checked against its end and every write against H (W C + 1) bytes: whatever is wrong with stream k comes back as status_dev[k], an
 * r2l_png_status; such a picture is unspecified (and in bounds) and the others are not disturbed.  Nothing is allocated or copied
 * and the host does not wait; no atomics: the same streams give the same bytes, and a picture does not depend on the other streams.
 * H and W from 1 to 16384, n_img up to 65535, offsets_dev 8-byte, status_dev 4-byte, workspace_dev 16-byte aligned, a workspace of
 * r2l_png_decode_workspace_bytes (a negative code on a bad argument; host only): R2L_EINVAL otherwise, before a device is touched.
 * n_img = 0 is a no-op.  The offsets are trusted as the pointers are: ascending, a stream shorter than 2 GiB. */
enum r2l_png_status {
    R2L_PNG_OK = 0,
    R2L_PNG_TRUNCATED = 1,      /* the stream ends inside a header, a block or the Adler-32 */
    R2L_PNG_BAD_HEADER = 2,     /* not a zlib header: method, window, check bits, or a preset dictionary */
    R2L_PNG_BAD_BLOCK = 3,      /* block type 3 */
    R2L_PNG_BAD_STORED = 4,     /* a stored block whose NLEN is not the complement of LEN */
    R2L_PNG_OVERSUBSCRIBED = 5, /* code lengths that claim more codes than there are */
    R2L_PNG_INCOMPLETE = 6,     /* code lengths that leave codes unused (other than a single code of one bit) */
    R2L_PNG_BAD_LENGTHS = 7,    /* too many lengths, a repeat with nothing to repeat or past the end, no end-of-block code */
    R2L_PNG_BAD_CODE = 8,       /* bits that are no symbol of the code, or a symbol deflate does not define */
    R2L_PNG_FAR_DISTANCE = 9,   /* a match that starts before the first byte of the output */
    R2L_PNG_TOO_LONG = 10,      /* more bytes than the image needs */
    R2L_PNG_TOO_SHORT = 11,     /* fewer */
    R2L_PNG_BAD_FILTER = 12,    /* a row whose filter byte is above 4 */
    R2L_PNG_BAD_ADLER = 13,     /* the Adler-32 of the bytes is not the stream's */
    R2L_PNG_BAD_OFFSETS = 14    /* offsets that do not ascend, or a stream of 2 GiB or more */
};
long long r2l_png_decode_workspace_bytes(int n_img, int H, int W, int C);
int r2l_png_decode(const unsigned char* zstreams_dev, const long long* offsets_dev, int n_img, int H, int W, int C, void* workspace_dev,
                   long long workspace_bytes, unsigned char* out_dev, int* status_dev, void* stream);

/* ---- training of the NeRF teacher (csrc/nerf_train.hip; host mirror: efficient-nerf_amd/train_teacher.py) ----
 * A teacher step is the launches above (layers, embedding, scans, loss, Adam) plus the backward pass of nerf_raw2outputs[_noise]:
 * g_raw_dev [n,S,4] from g_rgb_map_dev [n,3], the only output the losses reach (main.py:728 detaches z_samples).  raw [n,S,4],
 * z [n,S] per ray, rays_d [n,3], noise_dev [n,S] or NULL: the forward call's.  Division-free (a saturated sample, alpha = 1,
 * leaves 1e-10 in the transmittance product; nothing divides by it), any S >= 1, no atomics: the same inputs give the same bits.
 * The density gradient is exactly 0 where the relu is closed and on a last sample whose exp(-sigma 1e10) is 0.  g_raw_dev must
 * not overlap raw_dev; both 16-byte aligned.  With n = 0 the buffers may be NULL. */
int nerf_train_raw2outputs_backward(const float* raw_dev, const float* z_dev, const float* rays_d_dev, const float* noise_dev, int n,
                                    int S, int white_bkgd, const float* g_rgb_map_dev, float* g_raw_dev, void* stream);

/* A step's rays of the reference's use_batching loop (main.py:1137-1162, 1199-1210) without its ray bank: ray k of the step is pixel
 * order_dev[k] = image * H * W + row * W + column (int64, device; the caller's permutation already offset to the step's window) of
 * images_dev uint8 [n_img, H, W, 3] under poses_dev float32 [n_img, 3, 4].  Four contiguous [rows, 3] float32 outputs, the layout
 * the trainer reads: rays_o / rays_d are r2l_rays_from_images' (three channels, full resolution) and, with ndc != 0, nerf_ndc_rays
 * (H, W, focal, near_) of them, bit for bit; viewdirs (may be NULL) is rays_d / ||rays_d|| of the WORLD direction in either mode
 * (main.py:148-162); target is bytes / 255.  An index outside [0, n_img * H * W) gives NaN rows; rows = 0 launches nothing.  One
 * thread per ray, plain coalesced stores, no atomics: the same inputs give the same bits.  poses and the outputs 4-byte aligned,
 * order 8-byte aligned. */
int nerf_train_batch_rays(const unsigned char* images_dev, int n_img, int H, int W, const float* poses_dev, double focal,
                          const long long* order_dev, long long rows, int ndc, float near_, float* rays_o_dev, float* rays_d_dev,
                          float* viewdirs_dev, float* target_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* R2L_HIP_H */
