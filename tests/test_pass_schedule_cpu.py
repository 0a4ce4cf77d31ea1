"""engine.pass_schedule, the issue order of a pass as data, on the CPU: the 2D DualDecoder (mcnet) and the residual DualDecoder3d programs in
the three decoder modes, both directions.  (What the schedule turns into on the device is pinned by tests/test_issue_order_gpu.py.)"""
import pytest

from chap_amd import engine as E


def _program(which):
    from chap_amd.networks import DualDecoder, DualDecoder3d
    if which == "2d":
        return DualDecoder(1, 4, {"decoder_type": "mcnet"})._exec.prog
    return DualDecoder3d(n_channels=1, n_classes=2, normalization="batchnorm", has_dropout=True, has_residual=True)._exec.prog


@pytest.fixture(scope="module", params=["2d", "3d_residual"])
def prog(request):
    return _program(request.param)


def _ops(steps):
    return [op for _, lanes in steps for op in lanes]


@pytest.mark.parametrize("mode,side_decoder", [(E.GROUPED, 1), (E.FORKED, 1), (E.FORKED, 2), (E.SERIAL, 1)])
def test_forward_and_backward_order(prog, mode, side_decoder):
    fwd = E.pass_schedule(prog, mode, side_decoder, backward=False)
    bwd = E.pass_schedule(prog, mode, side_decoder, backward=True)
    trunk = [op for op in prog.ops if op.branch == 0]
    dec = {b: [op for op in prog.ops if op.branch == b] for b in (1, 2)}
    assert len(trunk) + len(dec[1]) + len(dec[2]) == len(prog.ops) and dec[1] and dec[2]
    for steps, rev in ((fwd, False), (bwd, True)):
        flat = _ops(steps)
        order = (lambda ops_: ops_[::-1]) if rev else (lambda ops_: ops_)
        # every op exactly once
        assert len(flat) == len(prog.ops) and {id(op) for op in flat} == {id(op) for op in prog.ops}
        # forward: the trunk before the decoders; backward: the decoders before the trunk; the trunk in (reversed) program order, on the pass's own stream
        part = flat[len(flat) - len(trunk):] if rev else flat[:len(trunk)]
        assert [id(op) for op in part] == [id(op) for op in order(trunk)]
        assert all(where == E.OWN and len(lanes) == 1 for where, lanes in steps if lanes and lanes[0].branch == 0)
        # each decoder's ops keep their (reversed) program order
        for b in (1, 2):
            assert [id(op) for op in flat if op.branch == b] == [id(op) for op in order(dec[b])]
        dsteps = [(where, lanes) for where, lanes in steps if not lanes or lanes[0].branch != 0]
        if mode == E.GROUPED:
            # the lockstep pairs are zip_branches' pairs, lane order kept, all on the pass's own stream
            pairs = E.zip_branches(dec[1], dec[2])
            assert [tuple(id(op) for op in lanes) for _, lanes in dsteps] == [tuple(id(op) for op in lanes) for lanes in order(pairs)]
            assert all(where == E.OWN for where, _ in dsteps) and any(len(lanes) == 2 for _, lanes in dsteps)
        elif mode == E.FORKED:
            # the forked decoder's ops all come before the other decoder's, in BOTH directions, then the join
            wheres = [where for where, _ in dsteps]
            n_fork = len(dec[side_decoder])
            assert wheres == [E.FORK] * n_fork + [E.OWN] * len(dec[3 - side_decoder]) + [E.JOIN]
            assert all(lanes[0].branch == side_decoder for where, lanes in dsteps if where == E.FORK)
            assert all(len(lanes) == 1 for where, lanes in dsteps if where != E.JOIN) and dsteps[-1][1] == ()
        else:
            assert all(where == E.OWN and len(lanes) == 1 for where, lanes in dsteps)
            assert [id(op) for op in flat] == [id(op) for op in order(list(prog.ops))]          # plain (reversed) program order
    if mode != E.FORKED:
        assert [tuple(id(op) for op in lanes) for _, lanes in bwd] == [tuple(id(op) for op in lanes) for _, lanes in fwd[::-1]]      # the exact reverse


def test_single_decoder_programs_run_in_program_order():
    from chap_amd.networks import UNet, VNet
    for m in (UNet(1, 4), VNet(n_channels=1, n_classes=2, normalization="batchnorm", has_dropout=True)):
        prog = m._exec.prog
        assert m._exec.nbranch <= 2
        assert [id(op) for op in _ops(E.pass_schedule(prog, E.SERIAL))] == [id(op) for op in prog.ops]
        assert [id(op) for op in _ops(E.pass_schedule(prog, E.SERIAL, backward=True))] == [id(op) for op in prog.ops[::-1]]


def test_executor_builds_a_schedule_once_and_reads_the_switches_live(monkeypatch):
    ex = E.Executor(None, _program("2d"))
    assert ex._schedule(E.GROUPED, False) is ex._schedule(E.GROUPED, False)
    assert [lanes for _, lanes in ex._schedule(E.GROUPED, False) if lanes[0].branch] == ex._zipped()
    monkeypatch.setenv("CHAP_SIDE_DECODER", "2")
    two = ex._schedule(E.FORKED, True)
    monkeypatch.setenv("CHAP_SIDE_DECODER", "1")
    one = ex._schedule(E.FORKED, True)
    assert two[0][1][0].branch == 2 and one[0][1][0].branch == 1


def test_switch_table_semantics(monkeypatch):
    names = ("CHAP_GROUP", "CHAP_SIDE_DECODER", "CHAP_C1_DIRECT", "CHAP_DEFER_WGRAD", "CHAP_SPLIT_CONCAT", "CHAP_FORK_MASK")
    assert sorted(E.SWITCHES) == sorted(names)
    for n in names:
        monkeypatch.delenv(n, raising=False)
    assert [E.switch(n) for n in names] == [1, 1, True, True, True, 14]
    for n, v, want in (("CHAP_GROUP", "0", 0), ("CHAP_GROUP", "3", 3), ("CHAP_SIDE_DECODER", "2", 2), ("CHAP_SIDE_DECODER", "02", 1), ("CHAP_SIDE_DECODER", "x", 1),
                       ("CHAP_C1_DIRECT", "0", False), ("CHAP_C1_DIRECT", "", True), ("CHAP_DEFER_WGRAD", "0", False), ("CHAP_DEFER_WGRAD", "off", True),
                       ("CHAP_SPLIT_CONCAT", "0", False), ("CHAP_SPLIT_CONCAT", "00", True), ("CHAP_FORK_MASK", "0", 0), ("CHAP_FORK_MASK", "15", 15)):
        monkeypatch.setenv(n, v)
        assert E.switch(n) == want, (n, v)
        monkeypatch.delenv(n)
    monkeypatch.setenv("CHAP_GROUP", "yes")
    with pytest.raises(ValueError):
        E.switch("CHAP_GROUP")
