"""The host-only planner probe shared by the CPU tests that ask chap_conv_fwd / chap_wgrad for their launch plans (tests/test_launch_plan_cpu.py,
tests/test_small_conv_cases_cpu.py, tests/test_k3_conv_cases_cpu.py): a small stand-alone program, built with the host compiler from chap_amd/csrc/conv_plan.h, wgrad_plan.h and
error.cpp, that reads request lines and prints one plan per line.  A helper module, not a conftest."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chap_amd", "csrc")

PROBE = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <string>
#include "conv_plan.h"
#include "wgrad_plan.h"
#include "error.cpp"

typedef std::map<std::string, std::string> kv;
static int geti(const kv& m, const char* k, int def = 0) { auto i = m.find(k); return i == m.end() ? def : atoi(i->second.c_str()); }
static char dummy[64];

static chap_src_t make_src(int C, int ld, int coff, int keep) {
    chap_src_t s;
    memset(&s, 0, sizeof(s));
    s.ptr = dummy; s.C = C; s.ld = ld; s.coff = coff; s.keep = keep ? (const uint8_t*)dummy : nullptr;
    return s;
}

int main() {
    char buf[4096];
    while (fgets(buf, sizeof(buf), stdin)) {
        std::istringstream in(buf);
        std::string op, tok;
        in >> op;
        kv m;
        while (in >> tok) { size_t e = tok.find('='); m[tok.substr(0, e)] = e == std::string::npos ? "" : tok.substr(e + 1); }
        if (op == "setenv") { for (auto& e : m) setenv(e.first.c_str(), e.second.c_str(), 1); continue; }
        if (op == "unsetenv") { for (auto& e : m) unsetenv(e.first.c_str()); continue; }
        const int st = geti(m, "s", 1), dims = geti(m, "dims", 2), sd = dims == 3 ? st : 1;
        if (op == "conv") {
            chap_conv_params p;
            memset(&p, 0, sizeof(p));
            p.nsrc = geti(m, "nsrc", 1); p.combine = geti(m, "combine");
            const int C0 = geti(m, "C0"), C1 = geti(m, "C1");
            p.src[0] = make_src(C0, geti(m, "ld0", C0), 0, geti(m, "keep0"));
            p.src[1] = make_src(C1, C1, 0, geti(m, "keep1"));
            if (geti(m, "cm0")) p.src[0].chan_mul = (const float*)dummy;
            if (geti(m, "cm1")) p.src[1].chan_mul = (const float*)dummy;
            p.N = geti(m, "N"); p.D = geti(m, "D", 1); p.H = geti(m, "H"); p.W = geti(m, "W");
            p.ksize = geti(m, "k"); p.stride = st; p.dims = dims;
            p.ID = p.D * sd; p.IH = p.H * st; p.IW = p.W * st;
            p.wpacked = dummy; p.out = dummy; p.Cout = geti(m, "Cout"); p.out_ld = (p.Cout + 3) / 4 * 4;
            p.out_mode = geti(m, "d2s"); p.out_Cn = geti(m, "Cn"); p.out_planar = geti(m, "planar"); p.out_f32 = geti(m, "f32out");
            p.stats = geti(m, "stats") ? (float*)dummy : nullptr; p.dtype = geti(m, "dtype", CHAP_BF16);
            conv_plan q;
            memset(&q, 0, sizeof(q));
            const int rc = conv_make_plan(&p, &q);
            static const char* routes[] = {"head", "wp", "kpar", "generic"};
            if (rc) printf("rc=%d error=%s\n", rc, chap_last_error());
            else printf("rc=0 route=%s geom=%d KC=%d GPT=%d NP=%d STEPS=%d nchunks=%d ntiles=%d NT=%d MR=%d cpar=%d\n", routes[q.route], q.geom,
                        q.b.KC, q.b.GPT, q.b.NP, q.b.STEPS, q.b.nchunks, q.b.ntiles, q.NT, q.MR, q.cpar);
        } else if (op == "wgrad") {
            chap_wgrad_params p;
            memset(&p, 0, sizeof(p));
            p.na = geti(m, "na", 1); p.combine = geti(m, "combine");
            const int C0 = geti(m, "C0"), C1 = geti(m, "C1"), Cb = geti(m, "Cb");
            p.a[0] = make_src(C0, C0, 0, geti(m, "keep0")); p.a[1] = make_src(C1, C1, 0, geti(m, "keep1")); p.b = make_src(Cb, Cb, 0, 0);
            if (geti(m, "cm0")) p.a[0].chan_mul = (const float*)dummy;
            if (geti(m, "cm1")) p.a[1].chan_mul = (const float*)dummy;
            p.N = geti(m, "N"); p.D = geti(m, "D", 1); p.H = geti(m, "H"); p.W = geti(m, "W");
            p.ksize = geti(m, "k"); p.stride = st; p.dims = dims;
            p.ID = p.D * sd; p.IH = p.H * st; p.IW = p.W * st;
            p.dtype = geti(m, "dtype", CHAP_BF16);
            wg_plan q;
            memset(&q, 0, sizeof(q));
            const int rc = wg_make_plan(&p, &q);
            if (rc) printf("rc=%d error=%s\n", rc, chap_last_error());
            else printf("rc=0 brick=%d KC=%d bn=%d mr=%d nsplit=%d Ca=%d Cb=%d taps=%d bytes=%zu ntiles=%ld\n", q.brick, q.KC, q.bn, q.mr, q.nsplit, q.Ca, q.Cb, q.taps, q.bytes, q.ntiles);
        } else if (op == "pack") {
            chap_pack_params p;
            memset(&p, 0, sizeof(p));
            p.kind = geti(m, "kind"); p.Cin = geti(m, "Cin"); p.Cout = geti(m, "Cout"); p.taps = geti(m, "taps"); p.dtype = geti(m, "dtype", CHAP_BF16);
            pack_geom g;
            conv_blocking b;
            const int rc = conv_pack_blocking(&p, "chap_pack_describe", &g, &b);
            if (rc) printf("rc=%d error=%s\n", rc, chap_last_error());
            else printf("rc=0 KC=%d GPT=%d NP=%d STEPS=%d nchunks=%d ntiles=%d\n", b.KC, b.GPT, b.NP, b.STEPS, b.nchunks, b.ntiles);
        } else {
            printf("rc=-99 error=unknown request\n");
        }
    }
    return 0;
}
"""

KNOBS = ["CHAP_CONV_WP", "CHAP_CONV_KPAR", "CHAP_CONV_KPAR_MAX", "CHAP_CONV_NT", "CHAP_CONV_MR", "CHAP_CONV_MINC", "CHAP_CONV_KC16_MAXC",
         "CHAP_CONV_KC16_MAXC2D", "CHAP_WGRAD_WP", "CHAP_WGRAD_WP_MR", "CHAP_WGRAD_BRICK", "CHAP_WGRAD_BLOCKS", "CHAP_WGRAD_BRICK_BLOCKS",
         "CHAP_WGRAD_WP_BLOCKS", "CHAP_WGRAD_TARGETS", "CHAP_WGRAD_BN16_MAXC"]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan_probe")
    (d / "probe.cpp").write_text(PROBE)
    exe = str(d / "probe")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC, str(d / "probe.cpp"), "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}

    def run(requests):
        """one fresh process per call (read-once knobs are read once per process): a list of request lines -> a list of dicts"""
        out = subprocess.run([exe], input="\n".join(requests) + "\n", env=env, check=True, capture_output=True, text=True).stdout.splitlines()
        res = []
        for line in out:
            rc, _, rest = line.partition(" ")
            d = {"rc": int(rc[3:])}
            if d["rc"]:
                d["error"] = rest[len("error="):]
            else:
                d.update((k, v if k == "route" else int(v)) for k, v in (t.split("=") for t in rest.split()))
            res.append(d)
        assert len(res) == sum(1 for r in requests if not r.startswith(("setenv", "unsetenv")))
        return res
    return run
