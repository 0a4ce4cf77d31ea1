"""Host side of the batched pass-B entry points, without a GPU: the ctypes mirrors of chap_mix_loss_multi_params and chap_bcpmix_params
against the header (sizes and the offsets the kernels depend on, via a compiled probe) and the argument errors, which are raised before
anything is launched."""
import ctypes
import os
import subprocess

import pytest

from chap_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ctypes_mirrors_match_the_header(tmp_path):
    probes = {"sizeof(chap_mix_loss_multi_params)": ctypes.sizeof(_lib.MixLossMultiParams),
              "offsetof(chap_mix_loss_multi_params, term)": _lib.MixLossMultiParams.term.offset,
              "sizeof(chap_bcpmix_params)": ctypes.sizeof(_lib.BcpMixParams),
              "offsetof(chap_bcpmix_params, mask)": _lib.BcpMixParams.mask.offset,
              "offsetof(chap_bcpmix_params, N)": _lib.BcpMixParams.N.offset,
              "offsetof(chap_bcpmix_params, D)": _lib.BcpMixParams.D.offset}
    c = tmp_path / "sz.c"
    body = "".join('printf("%%zu\\n", %s);\n' % e for e in probes)
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "chap_hip.h"\nint main(void){\n%sreturn 0;}\n' % body)
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == list(probes.values()), dict(zip(probes, out))
    assert ctypes.sizeof(_lib.MixLossMultiParams) == 8 + 4 * ctypes.sizeof(_lib.MixLossParams)


def _term(N=2, C=4, P=323, **kw):
    p = _lib.MixLossParams()
    p.logits, p.target_a, p.acc, p.loss, p.dlogits = 256, 256, 256, 256, 256      # never dereferenced: every call below fails its checks
    p.N, p.C, p.P = N, C, P
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _multi(*terms, nterms=None):
    m = _lib.MixLossMultiParams()
    m.nterms = len(terms) if nterms is None else nterms
    for i, t in enumerate(terms):
        m.term[i] = t
    return m


@pytest.mark.parametrize("entry", ["chap_mix_loss_multi_fwd", "chap_mix_loss_multi_bwd"])
def test_multi_term_argument_errors(entry):
    for m, what in ((_multi(nterms=0), "nterms"), (_multi(_term(), nterms=5), "nterms"), (_multi(_term(), _term(target_a=None)), "null argument in term 1"),
                    (_multi(_term(C=3)), "C=3"), (_multi(_term(), _term(P=322)), "common"), (_multi(_term(), _term(C=2)), "common"),
                    (_multi(_term(), _term(N=0)), "empty"), (_multi(_term(N=1 << 16, P=1 << 16)), "32-bit")):
        with pytest.raises(_lib.ChapError, match=what):
            _lib.call(entry, m, 0)
    with pytest.raises(_lib.ChapError, match="null argument in term 0"):
        _lib.call(entry, _multi(_term(loss=None, dlogits=None)), 0)


def test_bcp_mix_argument_errors():
    p = _lib.BcpMixParams()
    with pytest.raises(_lib.ChapError, match="null"):
        _lib.call("chap_bcp_mix", p, 0)
    for h in range(2):
        p.a[h], p.b[h], p.out[h], p.N[h] = 256, 256, 256, 1
    p.mask, p.box, p.Nm, p.H, p.W = 256, 256, 1, 0, 8
    with pytest.raises(_lib.ChapError, match="empty"):
        _lib.call("chap_bcp_mix", p, 0)
    p.H, p.W, p.D = 1 << 16, 1 << 16, 2
    with pytest.raises(_lib.ChapError, match="32-bit"):
        _lib.call("chap_bcp_mix", p, 0)
