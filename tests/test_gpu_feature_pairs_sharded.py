"""Every pair of problem features in the three point-sharded solves, on 2 and 3 ranks: forms 10 to 12 of the feature-pairs array
(tests/feature_pairs.py; forms 1 to 9: tests/test_gpu_feature_pairs.py) -- ea_solve_sharded (the host state machine),
ea_solve_sharded_device (the step kernel on the reduced sums) and ea_internal_solve_sharded_rows (the iteration kernel on the
reduced rows, the first choice of ea_solve_sharded_comm).  Gloo ranks share the one GPU (the harness of
tests/test_gpu_sharded.py); a rank builds its shard of a case (fp.shard_inputs through Built) under one of fp.SHARD_CUTS: even
halves, one full chunk beside a term of zero points, a one-point rank, a rank that holds nothing.  The workers assert nothing
about numbers: each writes what it saw, the parent compares with the composed long-double reference.

What is held, per run x cut x form: the 32 slots a rank sends at the first exchange against fp.shard_reference (no prior in
them; exact zeros from a rank without a valid row) and the reduced slots against the whole problem's sums of the points; q, t,
iteration count, `why` and the cost trace bit-identical on all ranks, the number of exchanges the one the form documents; the
solve against fp.reference_solve with the case's own loss (an auto-scaled problem runs with its current a and keeps it), the
costs at both ends against the whole reference, prior included; a failed block that one rank sees ends every rank at its first
evaluation.  The rows form runs exactly where the case is of the plain kernel family and every rank holds a head point; elsewhere
every rank alike reports used == 0 with the pose untouched and goes on to the sums form, as ea_solve_sharded_comm does.

Bars (none is this module's own): those of tests/test_gpu_feature_pairs.py -- fp64 sums 1e-11 of the largest entry, fp32
border_band.bounds over the inputs summed; fp64 solves equal `why` and counts, poses within 1e-7; fp32 1e-4 rad / 1e-3 m.  Every
fp32 case also runs as its fp64 twin: several mistakes a sharded driver could make stay below the fp32 solve bars
(tests/test_feature_pairs_reference.py::test_the_sharded_comparisons_can_tell holds every run to a visible one).  Sharded against
unsharded has no bar: they differ in summation order, under which these problems move by up to 1e-9; the deviation from the
same solve on one rank is printed."""
import datetime
import os
import socket
import sys

import numpy as np
import pytest

from edge_alignment_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import border_band as bb  # noqa: E402
import feature_pairs as fp  # noqa: E402

pytestmark = pytest.mark.gpu
RUNS = fp.sharded_runs()
FORMS = ("host", "device", "rows")
FORM_NAME = {"host": "10 sharded host", "device": "11 sharded device", "rows": "12 sharded rows"}
WORLD2 = tuple(c for c, (w, _) in fp.SHARD_CUTS.items() if w == 2)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _start(case):
    q0, t0 = fp.poses(case, scaled=False)
    return q0[0], t0[0]


class _DeviceDoubles:
    """`count` doubles of device memory at `ptr` as an object torch can wrap"""

    def __init__(self, ptr, count):
        self.__cuda_array_interface__ = {"shape": (count,), "typestr": "<f8", "data": (ptr, False), "version": 2}


# ---- the workers ---------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, out_dir, cuts, forms):
    import torch
    import torch.distributed as dist
    torch.cuda.init()  # before libea_hip touches the device
    from edge_alignment_amd import capi
    import test_gpu_feature_pairs as tg
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=60))
    dev = torch.device("cuda", 0)   # every rank shares the one GPU of the test box
    sums = torch.zeros(32, dtype=torch.float64, device=dev)
    seen = {}   # what the exchange carried the first time it was called: the 32 slots before and after the reduce

    def note(before, after):
        seen["n"] = seen.get("n", 0) + 1
        if seen["n"] == 1:
            seen["before"], seen["after"] = before, after

    def host_exchange(a):   # ea_solve_sharded: 32 host doubles
        before = a.copy()
        h = torch.from_numpy(a.copy())
        dist.all_reduce(h, op=dist.ReduceOp.SUM)
        a[:] = h.numpy()
        note(before, a.copy())

    def device_exchange(stream):   # ea_solve_sharded_device: gloo has no device path, staged under a stream synchronisation
        with torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=dev)):
            h = sums.cpu()
            before = h.numpy().copy()
            dist.all_reduce(h, op=dist.ReduceOp.SUM)
            sums.copy_(h)
            note(before, h.numpy().copy())

    def rows_exchange(ptr, count, stream):   # the rows form: the test folds the rows in float64
        assert count % 32 == 0
        with torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=dev)):
            rows = torch.as_tensor(_DeviceDoubles(ptr, count), device=dev)
            h = rows.cpu()
            before = h.numpy().reshape(-1, 32).sum(axis=0)
            dist.all_reduce(h, op=dist.ReduceOp.SUM)
            rows.copy_(h)
            note(before, h.numpy().reshape(-1, 32).sum(axis=0))

    def agree(vals):
        tt = torch.tensor(vals, dtype=torch.int32)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        return [int(tt[0]), int(tt[1])]

    out = {}
    for cut in cuts:
        for i, (kind, case) in enumerate(RUNS):
            b = tg.Built(capi, case, inputs=fp.shard_inputs(fp.host_inputs(case), cut, rank, case))
            try:
                q0, t0 = _start(case)
                for form in forms:
                    seen.clear()
                    rec = {}
                    if form == "host":
                        q, t, s = b.P.solve_sharded(q0, t0, host_exchange)
                    elif form == "device":
                        q, t, s = b.P.solve_sharded_device(q0, t0, device_exchange, sums.data_ptr(), solve_timeout_ms=20000.0)
                    else:
                        q, t, s, used = b.P.solve_sharded_rows(q0, t0, rows_exchange, agree, solve_timeout_ms=20000.0)
                        rec.update(used=used, back_q=q, back_t=t, rows_calls=seen.get("n", 0))
                        if not used:   # as ea_solve_sharded_comm goes on: the sums form
                            seen.clear()
                            q, t, s = b.P.solve_sharded_device(q0, t0, device_exchange, sums.data_ptr(), solve_timeout_ms=20000.0)
                    kl, al = b.P.get_loss()
                    rec.update(q=q, t=t, it=s["num_iterations"], why=s["why"], termination=s["termination"], it_cost=s["it_cost"],
                               initial_cost=s["initial_cost"], final_cost=s["final_cost"], calls=seen["n"], before=seen["before"],
                               after=seen["after"], loss=np.array([kl, al]))
                    out.update({"%s|%d|%s|%s" % (cut, i, form, k): v for k, v in rec.items()})
            finally:
                b.close()
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
    dist.barrier()
    dist.destroy_process_group()


# ---- the parent's comparisons ----------------------------------------------------------------------------------------------
def _slots(a):
    """the 32 accumulator slots -> cost, JtJ 6 x 6, Jtr (ea_types.h: the JtJ upper triangle row by row, Jtr, cost, invalid)"""
    JtJ, k = np.zeros((6, 6)), 0
    for i in range(6):
        for j in range(i, 6):
            JtJ[i, j] = JtJ[j, i] = a[k]
            k += 1
    return dict(cost=float(a[27]), JtJ=JtJ, Jtr=np.array(a[21:27]))


def _points(ref):
    return dict(cost=ref["cost_points"], JtJ=ref["JtJ_points"], Jtr=ref["Jtr_points"])


def _check_slots(worst, got, ref, bar, where):
    assert got[28] == ref["n_invalid"] and not got[29:].any(), (where, got[28:])
    if bar == 0.0:   # nothing that could round: exact zeros
        assert not got[:28].any() and not np.asarray(ref["cost_points"]) and not np.asarray(ref["JtJ_points"]).any(), where
    else:
        worst.add(bb.dev_sums(_slots(got), _points(ref)), bar, where)


def _one_rank(hip, tg, case):
    """the same solve on one rank (the all-reduce is the identity): information only"""
    b = tg.Built(hip, case)
    try:
        q, t, _ = b.P.solve_sharded(*_start(case), lambda a: None)
        return q, t
    finally:
        b.close()


def _compare(hip, tmp_path, cuts, forms, worst, worst_solve):
    """worst: the sums of the first exchange and the costs; worst_solve: the poses.  -> the set of `used` the rows form reported"""
    import test_gpu_feature_pairs as tg
    world = fp.SHARD_CUTS[cuts[0]][0]
    R = [np.load(tmp_path / ("rank%d.npz" % r)) for r in range(world)]
    used_seen, info = set(), [0.0, 0.0]
    for i, (kind, case) in enumerate(RUNS):
        inputs = fp.host_inputs(case)
        key = ("sharded", kind) + tuple(case[n] for n in fp.NAMES) + (case["seed"], case["index"])
        f64 = case["dtype"] == "f64"
        q0, t0 = _start(case)
        whole = fp.reference(case, q0, t0, np.longdouble, inputs, key=key)
        bars = dict(sums=1e-11) if f64 else fp.tolerances(case, q0, t0, inputs, key=key)
        want = fp.reference_solve(case, q0, t0, np.longdouble, inputs, auto=False, key=key) if kind != "failed" else None
        alone = _one_rank(hip, tg, case) if kind != "failed" else None
        for cut in cuts:
            ranges = fp.shard_ranges(inputs, cut, case)
            shard = [fp.shard_reference(case, q0, t0, np.longdouble, inputs, cut, r, key=key) for r in range(world)]
            # (a shard without a valid row -- no points, or the failed block alone -- has nothing that could round: a bar of 0)
            valid = [bool((~np.isnan(shard[r]["r"].astype(np.float64))).any()) for r in range(world)]
            sbar = [0.0 if not valid[r] else 1e-11 if f64 else fp.shard_tolerances(case, q0, t0, inputs, cut, r, key=key)["sums"] for r in range(world)]
            for form in forms:
                g = [{k: R[r]["%s|%d|%s|%s" % (cut, i, form, k)] for k in
                      ("q", "t", "it", "why", "termination", "it_cost", "initial_cost", "final_cost", "calls", "before", "after", "loss")
                      + (("used", "back_q", "back_t", "rows_calls") if form == "rows" else ())} for r in range(world)]
                where = "%s %s %s %s" % (case.name(), kind, cut, form)
                ran = form
                if form == "rows":
                    plain = not fp.is_variant(case) and all(ranges[r][0][1] > ranges[r][0][0] for r in range(world))
                    assert all(int(x["used"]) == (1 if plain else 0) for x in g), (where, [int(x["used"]) for x in g])
                    used_seen.add(int(g[0]["used"]))
                    if not plain:   # nothing was solved, nothing exchanged: the pose comes back as it went in
                        assert all(x["back_q"].tobytes() == q0.tobytes() and x["back_t"].tobytes() == t0.tobytes() and x["rows_calls"] == 0 for x in g), where
                        ran = "device"
                # the first exchange: what each rank sends, and what comes back
                for r in range(world):
                    _check_slots(worst, g[r]["before"], shard[r], sbar[r], "%s rank %d sends" % (where, r))
                    if not len(shard[r]["r"]):
                        assert not g[r]["before"].any(), (where, r, "a rank that holds nothing sends zeros")
                    _check_slots(worst, g[r]["after"], whole, bars["sums"], "%s rank %d receives" % (where, r))
                    assert g[r]["after"].tobytes() == g[0]["after"].tobytes(), (where, r, "the reduced slots")
                # lockstep
                for x in g[1:]:
                    for k in ("q", "t", "it", "why", "termination", "it_cost", "calls", "initial_cost", "final_cost"):
                        assert x[k].tobytes() == g[0][k].tobytes(), (where, k, x[k], g[0][k])
                x = g[0]
                assert int(x["calls"]) == int(x["it"]) + {"host": 1, "device": 2, "rows": 3}[ran], (where, int(x["calls"]), int(x["it"]))
                # an auto-scaled problem runs with its current a and keeps it
                assert all(tuple(y["loss"]) == tuple(map(float, fp.LOSS[case["loss"]])) for y in g), (where, [tuple(y["loss"]) for y in g])
                s = dict(why=str(x["why"]), num_iterations=int(x["it"]), termination=int(x["termination"]))
                if kind == "failed":   # the rank that cannot see the failed block ends with the one that can
                    assert whole["n_invalid"] == 1 and sorted(e["n_invalid"] for e in shard) == [0] * (world - 1) + [1], where
                    assert s == dict(why="initial_eval_failed", num_iterations=0, termination=hip.FAILURE), (where, s)
                    assert all(y["q"].tobytes() == q0.tobytes() and y["t"].tobytes() == t0.tobytes() for y in g), where
                    continue
                tg._check_solve(worst_solve, case, (x["q"], x["t"], s), want, where)
                held = fp.HELD[case["held"]]
                assert all(np.float64(x["t"][j]).tobytes() == np.float64(t0[j]).tobytes() for j in range(3) if held[3 + j]), (where, "held t")
                assert not all(held[:3]) or x["q"].tobytes() == q0.tobytes(), (where, "held q")
                end = fp.reference(case, x["q"], x["t"], np.longdouble, inputs, key=key)
                worst.add(bb.dev_rel(float(x["initial_cost"]), whole["cost"]), bars["sums"], where + " initial cost")
                worst.add(bb.dev_rel(float(x["final_cost"]), end["cost"]), bars["sums"], where + " final cost")
                if f64:
                    info[0] = max(info[0], synth.rotation_angle_between(x["q"], alone[0]))
                    info[1] = max(info[1], float(np.linalg.norm(x["t"] - alone[1])))
    print("FEATURE-PAIRS-GPU %-26s against the same fp64 solves on one rank (no bar): within %.2e rad, %.2e m" % ((worst_solve.form,) + tuple(info)))
    return used_seen


def _run(hip, tmp_path, cuts, forms, name):
    import torch.multiprocessing as mp
    import test_gpu_feature_pairs as tg
    world = fp.SHARD_CUTS[cuts[0]][0]
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), cuts, forms), nprocs=world, join=True)
    with tg.Worst(name + " sums") as worst, tg.Worst(name + " solve") as worst_solve:
        return _compare(hip, tmp_path, cuts, forms, worst, worst_solve)


def test_form10_solve_sharded(hip, tmp_path):
    _run(hip, tmp_path, WORLD2, ("host",), FORM_NAME["host"])


def test_form11_solve_sharded_device(hip, tmp_path):
    _run(hip, tmp_path, WORLD2, ("device",), FORM_NAME["device"])


def test_form12_solve_sharded_rows(hip, tmp_path):
    assert _run(hip, tmp_path, WORLD2, ("rows",), FORM_NAME["rows"]) == {0, 1}


def test_forms10_to_12_empty_rank(hip, tmp_path):
    """three ranks, the middle one without a point of any term: it sends zeros, receives the whole problem's sums and walks the
    solve with the others; the rows form finds a rank whose shard does not qualify and every rank falls back alike"""
    assert WORLD2 == ("even2", "chunk2", "lone2") and fp.SHARD_CUTS["empty3"][0] == 3
    assert _run(hip, tmp_path, ("empty3",), FORMS, "10-12 empty3") == {0}
