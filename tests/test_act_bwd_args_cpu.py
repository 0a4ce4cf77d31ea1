"""chap_act_bwd_reduce / _apply address every tensor with a 32-bit byte offset from its base: the entry points refuse, before any launch,
a tensor of 4 GB or more (the widest pixel stride among raw, the incoming gradients and the dense masks times the pixel count)."""
import pytest


def _params(L, **kw):
    p = L.ActBwdParams()
    p.r.ptr, p.r.C, p.r.ld = 64, 16, 16                    # 64 stands for 'not null': no check dereferences a pointer on the host
    p.g[0], p.g_ld[0], p.ng = 64, 16, 1
    p.gout, p.N, p.D, p.H, p.W, p.dtype = 64, 1, 1, 8, 8, L.BF16
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_four_gigabytes_are_refused_without_a_launch():
    from chap_amd import _lib as L
    # 2^27 pixels of 16 bf16 channels = 4 GB
    with pytest.raises(L.ChapError, match="chap_act_bwd.*4 GB"):
        L.call("chap_act_bwd_apply", _params(L, N=1 << 7, D=1 << 4, H=1 << 8, W=1 << 8), 0)
    # the wide buffer of a concat slice counts with its own stride: 2^26 pixels, ld = 32
    p = _params(L, N=1 << 6, D=1 << 4, H=1 << 8, W=1 << 8)
    p.g_ld[0], p.g_coff[0] = 32, 16
    with pytest.raises(L.ChapError, match="chap_act_bwd.*4 GB"):
        L.call("chap_act_bwd_apply", p, 0)
    # fp32 halves the pixel count
    with pytest.raises(L.ChapError, match="chap_act_bwd.*4 GB"):
        L.call("chap_act_bwd_apply", _params(L, N=1 << 6, D=1 << 4, H=1 << 8, W=1 << 8, dtype=L.F32), 0)
