"""Generates tests/golden/decode_shifts_d1.npz in the BUILD CONTAINER (needs /root/reference).

The reference's UNet5 (models/v0/net_definitions_torch.py) is imported UNCHANGED from /root/reference on top of this
repo's `open3d.ml.torch` facade, its decoder tensors are set to those of asr_hip.synth.make_weights(1, seed), and
decode_with_gradient(shifts, code) (:668-686) is recorded for 2 048 seeded (code, shift) pairs: 512 code rows, four
shifts each (the `rows` array), shifts uniform in +-1.5 so that some lie outside their voxel.  The fixture pins the
decoder at shifts and its hand-written backward pass (z3 -> z2 -> z1) against the reference implementation.

Stored: code [512,32], rows int32 [2048], shifts [2048,3], the five dense_decoder tensors, values [2048,2] and
grad [2048,3] (= z1[:, :3]).

usage: python tests/golden/make_decode_fixture.py
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "adaptive-surface-reconstruction_amd"))
sys.path.insert(0, REPO)
sys.path.insert(0, "/root/reference")

import open3d.ml.torch  # noqa: E402,F401  (this repo's facade: the layers UNet5 is built from)
from asr_hip import synth  # noqa: E402
from models.v0.net_definitions_torch import UNet5  # noqa: E402  (reference, unchanged)

SEED = 11
NAMES = ("dense_decoder1.weight", "dense_decoder1.bias", "dense_decoder2.weight", "dense_decoder2.bias",
         "dense_decoder3.weight")


def main():
    weights = synth.make_weights(1, seed=SEED)
    model = UNet5(channel_div=1, with_importance="all", normalized_channels=8, residual_skip_connection=True).eval()
    sd = model.state_dict()
    for name in NAMES:
        assert tuple(sd[name].shape) == weights[name].shape, (name, sd[name].shape, weights[name].shape)
        sd[name].copy_(torch.from_numpy(weights[name]))
    c = weights["dense_decoder1.weight"].shape[1] - 3
    rng = np.random.default_rng(SEED)
    code = rng.standard_normal((512, c)).astype(np.float32)
    rows = np.repeat(np.arange(512, dtype=np.int32), 4)
    shifts = rng.uniform(-1.5, 1.5, size=(len(rows), 3)).astype(np.float32)
    with torch.no_grad():
        values, grad = model.decode_with_gradient(torch.from_numpy(shifts), torch.from_numpy(code[rows]))
    out = {"code": code, "rows": rows, "shifts": shifts, "values": values.numpy().astype(np.float32),
           "grad": grad.numpy().astype(np.float32)}
    for name in NAMES:
        out[name] = weights[name]
    path = os.path.join(REPO, "tests", "golden", "decode_shifts_d1.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes): |values| max %.3g, |grad| max %.3g" % (path, os.path.getsize(path),
                                                                     np.abs(out["values"]).max(),
                                                                     np.abs(out["grad"]).max()))


if __name__ == "__main__":
    main()
