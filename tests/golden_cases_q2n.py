"""Cases of the Q2n fixtures (tests/golden/q2n_*.npz): shapes, block geometry and the seeded integer-valued images.  tools/make_golden.py --only q2n
builds the images from here and writes them into the fixtures together with the expected block maps; the tests read the fixtures only.

Every image is integer-valued (uint16 counts) so that the rounding of the native quantisation and the truncation of the Python port agree on it."""
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (name, B, C, H, W, block, shift)
CASES = [
    ("q2n_c1_64", 1, 1, 64, 64, 32, 32),
    ("q2n_c2_64", 1, 2, 64, 64, 32, 32),
    ("q2n_c4_64", 1, 4, 64, 64, 32, 32),
    ("q2n_c8_64", 1, 8, 64, 64, 32, 32),
    ("q2n_c3_64", 1, 3, 64, 64, 32, 32),       # zero-padded to 4 bands
    ("q2n_c6_64", 1, 6, 64, 64, 32, 32),       # zero-padded to 8 bands
    ("q2n_c4_63", 1, 4, 63, 63, 32, 32),       # one replicated row / column
    ("q2n_c4_70x90", 1, 4, 70, 90, 32, 32),    # 26 replicated rows, 6 replicated columns
    ("q2n_c4_48_s16", 1, 4, 48, 48, 32, 16),   # overlapping blocks, the last ones half replicated
    ("q2n_c8_40x48_b16s8", 1, 8, 40, 48, 16, 8),
    ("q2n_c4_48_b2", 2, 4, 48, 48, 32, 32),    # a batch of two different images
]
PAIRS = ("identical", "noise", "gain", "unrelated")
DEGENERATE = ("q2n_degenerate", 1, 4, 64, 64, 32, 32)  # blocks: (0,0) both constant, (0,1) gt band 2 constant, (1,0) gt all zero, (1,1) regular
N_PERMUTATIONS = 8


def path(name):
    return os.path.join(GOLDEN_DIR, name + ".npz")


def load(name):
    with np.load(path(name)) as z:
        return {k: z[k] for k in z.files}


def _scene(rng, B, C, H, W, phase):
    """smooth bands + texture + noise, in counts: every 16 x 16 block of every band varies by far more than one count"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((B, C, H, W))
    for b in range(B):
        for k in range(C):
            base = 400.0 + 60.0 * k + 3.0 * x + 2.0 * y
            wave = 220.0 * np.sin(2 * np.pi * (x / 23.0 + k / 5.0 + phase + 0.3 * b)) * np.cos(2 * np.pi * (y / 31.0 + phase))
            out[b, k] = base + wave + rng.normal(0.0, 15.0, (H, W))
    return np.clip(np.rint(out), 0, 65535).astype(np.uint16)


def images(case):
    """gt (B, C, H, W) uint16 and {pair: pred} of one case"""
    name, B, C, H, W, _, _ = case
    rng = np.random.RandomState(1000 + sum(ord(ch) for ch in name))
    gt = _scene(rng, B, C, H, W, 0.0)
    g = gt.astype(np.float64)
    preds = {
        "identical": gt.copy(),
        "noise": np.clip(np.rint(g + rng.normal(0.0, 25.0, g.shape)), 0, 65535).astype(np.uint16),
        "gain": np.rint(0.8 * g).astype(np.uint16),
        "unrelated": _scene(rng, B, C, H, W, 0.37),
    }
    return gt, preds


def degenerate_images():
    name, B, C, H, W, block, _ = DEGENERATE
    rng = np.random.RandomState(77)
    gt = _scene(rng, B, C, H, W, 0.0)
    pred = np.clip(np.rint(gt.astype(np.float64) + rng.normal(0.0, 25.0, gt.shape)), 0, 65535).astype(np.uint16)
    gt[:, :, :block, :block] = 500            # (0, 0): both images constant and equal -> T3 == 0, bias == 1
    pred[:, :, :block, :block] = 500
    gt[:, 2, :block, block:] = 700            # (0, 1): one gt band constant -> t = 1e-8
    gt[:, :, block:, :block] = 0              # (1, 0): gt all zero -> s == 0, the branch without a division
    return gt, {"noise": pred}
