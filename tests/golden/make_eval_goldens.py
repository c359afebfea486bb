"""Generates tests/golden/eval_psnr.npz by importing the REFERENCE's own calc_psnr (utils/slam_external.py:49-51,
the function eval() calls at utils/eval_helpers.py:483) from /root/reference (read-only) on the CPU, like
make_goldens.py.  Captured: two seeded 3x24x40 float32 images, a 0/1 mask, and calc_psnr of the masked pair
(the [3,1] per-channel values and their mean, as eval() forms it).  Only the data is committed.  Run:
    python tests/golden/make_eval_goldens.py
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    sys.path.insert(0, REF)
    ext = importlib.import_module("utils.slam_external")
    rng = np.random.RandomState(20240)
    gt_im = rng.rand(3, 24, 40).astype(np.float32)
    im = np.clip(gt_im + 0.05 * rng.randn(3, 24, 40), 0, 1).astype(np.float32)
    mask = (rng.rand(1, 24, 40) > 0.25)
    wi, wg = torch.from_numpy(im) * torch.from_numpy(mask), torch.from_numpy(gt_im) * torch.from_numpy(mask)
    per_channel = ext.calc_psnr(wi, wg)
    np.savez(os.path.join(OUT, "eval_psnr.npz"), im=im, gt_im=gt_im, mask=mask,
             psnr_per_channel=per_channel.numpy(), psnr=per_channel.mean().numpy())
    print("wrote eval_psnr.npz", float(per_channel.mean()))


if __name__ == "__main__":
    main()
