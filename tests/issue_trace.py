"""Issue-order recorder: what ONE training iteration hands to the runtime, in the order in which it is handed over.

Under capture the issue order is the creation order of the graph's nodes, by which the ROCm 7.2 graph executor places the chains on
its hardware queues ("Issue order": it alone moves a 2D step between 6.5 and 8.05 ms), and a lost join is a race
that the bit-identity tests may pass by luck.  So the record holds, one line each and in issue order:

    L <entry point> <stream> [g<region> l<lane>]     every _lib.call(name, params, stream) and _lib.pack_multi(...) (`chap_pack_multi`)
    GB <stream> g<region> / GN g<region> l<lane> / GE g<region>      begin, next_lane and end of an enabled _lib.group region
    WS <stream> <stream>   Stream.wait_stream        WE <stream> <event>   Stream.wait_event        ER <event> <stream>   Event.record

Streams and events are labelled by order of first appearance (s0, s1, ..., e0, ...), so a record does not depend on handles.  Torch's
own copies and fills (copy_, zero_, add_ on the seed word, the schedule-block upload) are not recorded, and neither are a launch's
parameters (CHAP_SPLIT_CONCAT=0 issues the same entry points as the default: its record equals 2d_eager's).  The recorder only observes:
every patched function calls through, and what was patched is restored in a `finally`.

An eager step() is recorded directly; a capture is recorded during capture(warmup=1) with the recording switched on for the captured
pass only (the warm-up is eager).  The four-graph data-parallel capture (ChapStep._capture_dp) needs RCCL and is left to the
bit-identity tests of tests/test_parallel_gpu.py.

`python -m tests.issue_trace DIR [case ...]` writes every case's full record to DIR/<case>.txt and the fixture lines (case name,
SHA-256 of the record, counts) to DIR/summary.txt; tests/golden/issue_order_parent.txt is such a summary, made on the commit BEFORE the
executor's and the training step's schedules were rewritten (tests/test_issue_order_gpu.py).
"""
import contextlib
import hashlib
import os
import sys

import torch

DEV = "cuda"


class Recorder:
    def __init__(self, only_capturing=False):
        self.lines, self.only_capturing = [], only_capturing
        self._streams, self._events, self._keep = {}, {}, []
        self._region, self._lane, self._nregions = None, 0, 0

    def _on(self):
        return not self.only_capturing or torch.cuda.is_current_stream_capturing()

    def _s(self, handle):
        handle = int(handle or 0)
        return self._streams.setdefault(handle, "s%d" % len(self._streams))

    def _e(self, event):
        if id(event) not in self._events:
            self._keep.append(event)            # (kept alive: the id of a freed event would be handed out again)
            self._events[id(event)] = "e%d" % len(self._events)
        return self._events[id(event)]

    def launch(self, name, stream):
        if self._on():
            where = "" if self._region is None else " g%d l%d" % (self._region, self._lane)
            self.lines.append("L %s %s%s" % (name, self._s(stream), where))

    @contextlib.contextmanager
    def recording(self):
        from chap_amd import _lib as L
        rec = self
        saved = (L.call, L.pack_multi, L.group.__enter__, L.group.next_lane, L.group.__exit__,
                 torch.cuda.Stream.wait_stream, torch.cuda.Stream.wait_event, torch.cuda.Event.record)
        call, pack_multi, g_enter, g_next, g_exit, wait_stream, wait_event, ev_record = saved

        def r_call(name, params, stream):
            rec.launch(name, stream)
            return call(name, params, stream)

        def r_pack_multi(entries, n, max_total, stream):
            rec.launch("chap_pack_multi", stream)
            return pack_multi(entries, n, max_total, stream)

        def r_enter(self):
            if self.enabled and rec._on():
                rec._region, rec._lane, rec._nregions = rec._nregions, 0, rec._nregions + 1
                rec.lines.append("GB %s g%d" % (rec._s(self.stream), rec._region))
            return g_enter(self)

        def r_next(self):
            if self.enabled and rec._region is not None:
                rec._lane += 1
                rec.lines.append("GN g%d l%d" % (rec._region, rec._lane))
            return g_next(self)

        def r_exit(self, et, ev, tb):
            if self.enabled and rec._region is not None:
                rec.lines.append("GE g%d" % rec._region)
                rec._region = None
            return g_exit(self, et, ev, tb)

        def r_wait_stream(self, stream):
            if rec._on():
                rec.lines.append("WS %s %s" % (rec._s(self.cuda_stream), rec._s(stream.cuda_stream)))
            return wait_stream(self, stream)

        def r_wait_event(self, event):
            if rec._on():
                rec.lines.append("WE %s %s" % (rec._s(self.cuda_stream), rec._e(event)))
            return wait_event(self, event)

        def r_record(self, stream=None):
            if rec._on():
                st = torch.cuda.current_stream() if stream is None else stream
                rec.lines.append("ER %s %s" % (rec._e(self), rec._s(st.cuda_stream)))
            return ev_record(self, stream)

        try:
            L.call, L.pack_multi = r_call, r_pack_multi
            L.group.__enter__, L.group.next_lane, L.group.__exit__ = r_enter, r_next, r_exit
            torch.cuda.Stream.wait_stream, torch.cuda.Stream.wait_event, torch.cuda.Event.record = r_wait_stream, r_wait_event, r_record
            yield self
        finally:
            (L.call, L.pack_multi, L.group.__enter__, L.group.next_lane, L.group.__exit__,
             torch.cuda.Stream.wait_stream, torch.cuda.Stream.wait_event, torch.cuda.Event.record) = saved

    def text(self):
        return "\n".join(self.lines) + "\n"


def counts(text):
    """The counts of a record: launches, grouped regions, launches per stream label, waits, event records."""
    lines = text.splitlines()
    per = {}
    for ln in lines:
        if ln.startswith("L "):
            s = ln.split()[2]
            per[s] = per.get(s, 0) + 1
    return dict(launches=sum(per.values()), regions=sum(ln.startswith("GB ") for ln in lines),
                streams=",".join("%s:%d" % (s, per[s]) for s in sorted(per, key=lambda s: int(s[1:]))),
                waits=sum(ln.startswith(("WS ", "WE ")) for ln in lines), records=sum(ln.startswith("ER ") for ln in lines))


def summary_line(name, text):
    c = counts(text)
    return "%s %s launches=%d regions=%d streams=%s waits=%d records=%d" % (
        name, hashlib.sha256(text.encode()).hexdigest(), c["launches"], c["regions"], c["streams"], c["waits"], c["records"])


def parse_summary_line(line):
    """one fixture line -> (sha256, {count name: text})"""
    _, sha, *kv = line.split()
    return sha, dict(x.split("=", 1) for x in kv)


def parse_summary(path):
    """fixture file -> {case: parse_summary_line(its line)}"""
    with open(path) as f:
        return {ln.split()[0]: parse_summary_line(ln) for ln in f if ln.strip()}


# ---------------------------------------------------------------------------------------------------------------- the cases
# name -> dict(net='2d' | '3d' | '3d_res', mode='eager' | 'captured', args=..., env=..., step='chap' | 'ablation', bf16=...)
CASES = {
    "2d_eager": dict(net="2d", mode="eager"),
    "2d_captured": dict(net="2d", mode="captured"),
    "3d_eager": dict(net="3d", mode="eager"),
    "3d_captured": dict(net="3d", mode="captured"),
    "2d_captured_single_stream": dict(net="2d", mode="captured", args=dict(concurrent=False)),
    "2d_captured_no_adv_noise": dict(net="2d", mode="captured", args=dict(adv_noise=False)),
    "2d_dropout_eager": dict(net="2d", mode="eager", args=dict(dropout=True)),
    "2d_dropout_captured": dict(net="2d", mode="captured", args=dict(dropout=True), fp_inject=True),
    "3d_residual_eager": dict(net="3d_res", mode="eager"),
    "3d_residual_captured": dict(net="3d_res", mode="captured"),
    "2d_ablation_eager": dict(net="2d", mode="eager", step="ablation"),
    "2d_captured_group0": dict(net="2d", mode="captured", env={"CHAP_GROUP": "0"}),
    "2d_captured_fork_mask15": dict(net="2d", mode="captured", env={"CHAP_FORK_MASK": "15"}),
    "2d_captured_fork_mask0": dict(net="2d", mode="captured", env={"CHAP_FORK_MASK": "0"}),
    "2d_eager_defer_wgrad0": dict(net="2d", mode="eager", env={"CHAP_DEFER_WGRAD": "0"}),
    "2d_eager_side_decoder2": dict(net="2d", mode="eager", env={"CHAP_SIDE_DECODER": "2"}),
    "2d_eager_split_concat0": dict(net="2d", mode="eager", env={"CHAP_SPLIT_CONCAT": "0"}),
    "2d_eager_bf16_c1_direct0": dict(net="2d", mode="eager", env={"CHAP_C1_DIRECT": "0"}, bf16=True),
}

_inputs = {}


def _net_inputs(net):
    """State, batch, injected randomness and box of tests/test_train_step_gpu.py::test_grouped_decoder_launches_equal_separate_launches
    (made once per process; nothing here changes them)."""
    key = "2d" if net == "2d" else "3d"
    if key not in _inputs:
        from oracle import init as oinit
        from oracle import train_step as ots
        from tests.iteration_parity import inject_2d, inject_3d, to_dev
        if key == "2d":
            B, lbs, sp = 8, 4, (64, 64)
            state = oinit.dual_decoder_2d_state(301)
            vol, lab = ots.synthetic_batch(1337, lbs, B - lbs, *sp)
            inj = to_dev(inject_2d(B - lbs, lbs // 2 + (B - lbs) // 2, sp[0], sp[1], 2), 2)
            inj["drop_F"] = to_dev({"drop_F": oinit.drop_masks_2d(11, B, sp[0], sp[1])}, 2)["drop_F"]      # AblationStep's full-batch pass
            box, extra = (7, 11), {}
        else:
            B, lbs, sp = 4, 2, (16, 32, 16)
            state = oinit.dual_decoder_3d_state(401)
            vol, lab = ots.synthetic_batch_3d(1337, lbs, B - lbs, *sp)
            inj = to_dev(inject_3d(B - lbs, lbs // 2 + (B - lbs) // 2, sp, 2), 3)
            box, extra = (2, 5, 3), {"num_classes": 2}
        _inputs[key] = dict(state=state, vol=vol.to(DEV), lab=lab.to(DEV), inj=inj, box=box, args=dict(dict(labeled_bs=lbs, batch_size=B, vat_iters=2), **extra))
    return _inputs[key]


@contextlib.contextmanager
def _environ(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def record_case(name):
    """Run one case on the GPU and return its full text record."""
    from chap_amd.networks import DualDecoder, DualDecoder3d
    from chap_amd.train import AblationStep, ChapStep
    case = CASES[name]
    inp = _net_inputs(case["net"])
    if case["net"] == "2d":
        m = DualDecoder(1, 4, {"decoder_type": "mcnet"})
    else:
        m = DualDecoder3d(n_channels=1, n_classes=2, normalization="batchnorm", has_dropout=True, has_residual=case["net"] == "3d_res")
    m = m.to(DEV).train()
    m.load_state_dict(inp["state"], strict=True)
    if case.get("bf16"):
        m.set_compute_dtype(torch.bfloat16)
    inj = dict(inp["inj"])
    if case.get("fp_inject"):       # no host copies under capture: the scripted draws of the perturbed pass on the device (tests/test_train_step_gpu.py:262-278)
        from oracle import filter_dropout as ofd
        _, scores, uniforms = ofd.fd_inputs(B=inp["vol"].shape[0] - inp["args"]["labeled_bs"])
        inj.update(fp_uniforms=[(a.to(DEV), b.to(DEV)) for a, b in uniforms], sim_score=[sc.to(DEV) for sc in scores])
    with _environ(case.get("env", {})):
        step = (AblationStep if case.get("step") == "ablation" else ChapStep)(m, dict(inp["args"], **case.get("args", {})))
        step.iter_num = 4500
        rec = Recorder(only_capturing=case["mode"] == "captured")
        with rec.recording():
            if case["mode"] == "eager":
                step.step(inp["vol"], inp["lab"], box_yx=inp["box"], inject=inj)
            else:
                step.capture(inp["vol"], inp["lab"], warmup=1, inject=inj)
        torch.cuda.synchronize()
    return rec.text()


def write_records(directory, names=None):
    """Every case's full record to `directory`/<case>.txt and the fixture lines to `directory`/summary.txt (returned)."""
    os.makedirs(directory, exist_ok=True)
    out = []
    for name in names or CASES:
        text = record_case(name)
        with open(os.path.join(directory, name + ".txt"), "w") as f:
            f.write(text)
        out.append(summary_line(name, text))
        print(out[-1], flush=True)
    with open(os.path.join(directory, "summary.txt"), "w") as f:
        f.write("\n".join(out) + "\n")
    return out


if __name__ == "__main__":
    write_records(sys.argv[1], sys.argv[2:] or None)
