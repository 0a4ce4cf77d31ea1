"""The host-only probe of the launch merging (chap_amd/csrc/launch.cpp), shared by tests/test_group_merge_cpu.py: a small stand-alone program with its own
main that includes launch.cpp and error.cpp and drives chap_group_begin / chap_group_record / chap_group_next_lane / chap_group_end / chap_group_cancel
directly.  Its chap_pending items carry a fake `merged` callback that logs what it is handed; it makes no HIP call and nothing touches a device.  Built
with hipcc and the host sanitizers (address, undefined) and run as a program.  A helper module, not a conftest.

Request lines (stdin), one answer line each unless noted:
  begin S                      chap_group_begin((void*)S)                                  -> `rc N`
  lane                         chap_group_next_lane()                                      -> `rc N`
  rec ID FN GX GY GZ BX LDS S  what chap_launch_ptr does with a launch on stream S: record it while recording (-> `rc N`), else issue it at once
                               (-> a `grid` line, then `rc N`)
  trec ID FN GX GY GZ BX LDS S the same from a second std::thread                           -> `thread recording=R`, then as `rec`
  failat K CODE                the K-th call of the callback from now (0-based) returns CODE (and is logged as every call is)
  end                          chap_group_end()                                            -> the `grid` lines, then `rc N [error text]`
  cancel                       chap_group_cancel()                                         -> `rc N`
  recording                    -> `recording R`
A grid line: `grid n=N stream=S fn=FN g=GX,GY,GZ b=BX lds=LDS items=ID:CHECKSUM,...` (geometry of the first item, as chap_launch_merged takes it).
An item's argument bytes are arg[i] = (ID * 131 + i * 7 + (ID >> 3)) & 255; CHECKSUM is the 32-bit FNV-1a hash of all sizeof(arg) bytes AS HANDED OVER."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chap_amd", "csrc")
ARG_BYTES = 768                                             # sizeof(chap_pending::arg), printed by the probe as its first line and compared
MAX_LANES = 4                                               # CHAP_MAX_LANES of the product build

PROBE = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <thread>
#include "launch.cpp"
#include "error.cpp"

static long g_calls = 0, g_fail_at = -1;
static int g_fail_code = 0;

static unsigned fnv(const unsigned char* p, size_t n) {
    unsigned h = 2166136261u;
    for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 16777619u; }
    return h;
}

static int fake_merged(const chap_pending* const* items, int n, hipStream_t s) {
    printf("grid n=%d stream=%ld fn=%ld g=%u,%u,%u b=%u lds=%u items=", n, (long)(size_t)s, (long)(size_t)items[0]->fn, items[0]->grid.x, items[0]->grid.y,
           items[0]->grid.z, items[0]->block.x, items[0]->lds);
    for (int i = 0; i < n; ++i) {
        int id;
        memcpy(&id, items[i]->name, sizeof(id));            // (the id travels in the name's storage, not in the argument bytes under test)
        printf("%s%d:%u", i ? "," : "", id, fnv(items[i]->arg, sizeof(items[i]->arg)));
    }
    printf("\n");
    const long k = g_calls++;
    return k == g_fail_at ? g_fail_code : CHAP_OK;
}

static int g_ids[1 << 16];
static int g_nids = 0;

static int do_rec(std::istringstream& in) {
    long id, fn, gx, gy, gz, bx, lds, s;
    in >> id >> fn >> gx >> gy >> gz >> bx >> lds >> s;
    if (g_nids >= (1 << 16)) { printf("rc -98 too many records\n"); return -98; }
    g_ids[g_nids] = (int)id;
    chap_pending p;
    p.fn = (const void*)(size_t)fn; p.grid = dim3((unsigned)gx, (unsigned)gy, (unsigned)gz); p.block = dim3((unsigned)bx); p.lds = (unsigned)lds;
    p.merged = &fake_merged; p.name = (const char*)&g_ids[g_nids++];
    for (size_t i = 0; i < sizeof(p.arg); ++i) p.arg[i] = (unsigned char)((id * 131 + (long)i * 7 + (id >> 3)) & 255);
    if (chap_group_recording()) return chap_group_record(p, (hipStream_t)(size_t)s);
    const chap_pending* one = &p;
    return fake_merged(&one, 1, (hipStream_t)(size_t)s);
}

int main() {
    printf("arg_bytes %zu max_lanes %d max_group %d\n", sizeof(chap_pending::arg), CHAP_MAX_LANES, CHAP_MAX_GROUP);
    char buf[512];
    while (fgets(buf, sizeof(buf), stdin)) {
        std::istringstream in(buf);
        std::string op;
        in >> op;
        if (op == "begin") { long s; in >> s; printf("rc %d\n", chap_group_begin((void*)(size_t)s)); }
        else if (op == "lane") printf("rc %d\n", chap_group_next_lane());
        else if (op == "rec") printf("rc %d\n", do_rec(in));
        else if (op == "trec") {
            int rc = 0;
            std::thread t([&] { printf("thread recording=%d\n", (int)chap_group_recording()); rc = do_rec(in); });
            t.join();
            printf("rc %d\n", rc);
        }
        else if (op == "failat") { long k; in >> k >> g_fail_code; g_fail_at = g_calls + k; printf("rc 0\n"); }
        else if (op == "end") { const int rc = chap_group_end(); if (rc < 0) printf("rc %d %s\n", rc, chap_last_error()); else printf("rc %d\n", rc); }
        else if (op == "cancel") printf("rc %d\n", chap_group_cancel());
        else if (op == "recording") printf("recording %d\n", (int)chap_group_recording());
        else if (op.empty()) continue;
        else printf("rc -99 unknown request\n");
        fflush(stdout);
    }
    return 0;
}
"""


def hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("group_probe")
    (d / "probe.cpp").write_text(PROBE)
    exe = str(d / "probe")
    subprocess.run([hipcc(), "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", CSRC, str(d / "probe.cpp"), "-o", exe],
                   check=True)      # (host code only: every sanitizer flag is -Xarch_host, which also reaches the host link)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")

    def run(requests):
        """one fresh process per call: request lines -> answer lines; a sanitizer report makes the program exit non-zero, which raises here"""
        r = subprocess.run([exe], input="\n".join(requests) + "\n", env=env, capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-2000:])
        out = r.stdout.splitlines()
        assert out[0] == "arg_bytes %d max_lanes %d max_group %d" % (ARG_BYTES, MAX_LANES, MAX_LANES), out[0]
        return out[1:]
    return run
