#!/usr/bin/env python
"""Entry point that trains the NeRF teacher with the reference's `main.py --model_name nerf --config configs/lego.txt` command
line; see efficient-nerf_amd/train_teacher.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pkg  # noqa: E402

_pkg.load()
from efficient_nerf_amd.train_teacher import main  # noqa: E402

if __name__ == '__main__':
    sys.exit(main())
