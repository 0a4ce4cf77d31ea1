#!/usr/bin/env python3
"""Writes tests/golden/vnet_residual_32.npz from the IMPORTED reference networks built with has_residual=True (ResidualConvBlock,
code/networks/vnet.py:37-67).  Runs on the CPU, where the reference tree is present; the reference is reached only through
oracle.gen_golden.import_reference().  What is written is data: a seeded input, seeds of the state-dict recipes (oracle/init.py, whose
BatchNorm running statistics are random, not the constructor's 0 / 1), logits and BatchNorm running statistics.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_residual.py

Contents (fp32): x [2, 1, 32, 32, 16]; state_seed (oracle.init.dual_decoder_3d_state), vnet_state_seed (oracle.init.vnet_state);
eval_logits0 / eval_logits1 (DualDecoder3d's heads) and vnet_eval_logits, whole; train-mode logits with has_dropout=False,
train_logits0_sub / train_logits1_sub / vnet_train_logits_sub = every second voxel per axis ([:, :, ::2, ::2, ::2]: the whole
tensors would take the file past the repository's 1 MiB limit); after_rm_<layer> / after_rv_<layer>: the running statistics of
DualDecoder3d after that one training-mode pass for BN_LAYERS, a last-stage layer (no ReLU behind it) and an ordinary one."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle import init as oinit  # noqa: E402
from oracle.gen_golden import import_reference  # noqa: E402

STATE_SEED, VNET_STATE_SEED, X_SEED = 211, 213, 23
BN_LAYERS = ("encoder.block_two.conv.4", "decoder1.block_six.conv.1")       # last stage of a residual block / first stage of one
OUT = os.path.join(ROOT, "tests", "golden", "vnet_residual_32.npz")


def _np(t):
    return t.detach().cpu().numpy().astype(np.float32)


def main():
    ref = import_reference()
    x = torch.rand(2, 1, 32, 32, 16, generator=torch.Generator().manual_seed(X_SEED))
    out = {"x": _np(x), "state_seed": STATE_SEED, "vnet_state_seed": VNET_STATE_SEED, "bn_layers": np.array(BN_LAYERS)}

    def build(cls, state):
        m = ref[cls](n_channels=1, n_classes=2, normalization="batchnorm", has_dropout=False, has_residual=True)
        plain = ref[cls](n_channels=1, n_classes=2, normalization="batchnorm", has_dropout=False, has_residual=False)
        assert list(m.state_dict().keys()) == list(plain.state_dict().keys())
        m.load_state_dict(state, strict=True)
        return m

    md = build("DualDecoder3d", oinit.dual_decoder_3d_state(STATE_SEED))
    mv = build("VNet", oinit.vnet_state(VNET_STATE_SEED))
    with torch.no_grad():
        md.eval(), mv.eval()
        o1, o2 = md(x)
        out["eval_logits0"], out["eval_logits1"], out["vnet_eval_logits"] = _np(o1), _np(o2), _np(mv(x))
        md.train(), mv.train()
        t1, t2 = md(x)
        tv = mv(x)
    sub = (slice(None), slice(None), slice(None, None, 2), slice(None, None, 2), slice(None, None, 2))
    out["train_logits0_sub"], out["train_logits1_sub"], out["vnet_train_logits_sub"] = _np(t1[sub]), _np(t2[sub]), _np(tv[sub])
    sd = md.state_dict()
    for k in BN_LAYERS:
        out["after_rm_" + k], out["after_rv_" + k] = _np(sd[k + ".running_mean"]), _np(sd[k + ".running_var"])
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes; |eval logits| max", float(o1.abs().max()), float(o2.abs().max()))


if __name__ == "__main__":
    main()
