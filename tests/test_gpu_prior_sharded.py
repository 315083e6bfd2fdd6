"""NormalPriors in the point-sharded solves, two gloo ranks on the one GPU (the harness of tests/test_gpu_sharded.py): every
rank sets the same prior, and each of the three forms -- ea_solve_sharded (host state machine), ea_solve_sharded_device
(step kernel on the reduced sums) and the rows exchange of ea_solve_sharded_comm (iteration kernel folding the reduced
rows) -- equals the unsharded prior solve.  Counted once per shard instead, the prior would weigh twice: the solve with a
doubled prior is shown to end elsewhere, so the comparison can tell the two apart."""
import os
import socket

import numpy as np
import pytest

from edge_alignment_amd import synth

pytestmark = pytest.mark.gpu
Q0, T0 = np.array([1.0, 0, 0, 0]), np.zeros(3)
_R = np.random.default_rng(11)
AQ, BQ = _R.normal(size=(3, 4)) * 40.0, np.array([0.999, 0.01, -0.02, 0.015])
AT, BT = _R.normal(size=(3, 3)) * 30.0, np.array([0.02, -0.02, 0.03])


def _problem():
    return synth.config_c2_twin(seed=17, n_points=30011)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _DeviceDoubles:
    def __init__(self, ptr, count):
        self.__cuda_array_interface__ = {"shape": (count,), "typestr": "<f8", "data": (ptr, False), "version": 2}


def _set(P, scale=1.0):
    P.set_normal_prior(0, AQ * scale, BQ)
    P.set_normal_prior(1, AT * scale, BT)


def _worker(rank, world, port, out_dir):
    import torch
    import torch.distributed as dist
    torch.cuda.init()
    from edge_alignment_amd import capi, dist as ead
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    cfg = _problem()
    n = cfg["xyz"].shape[0]
    cut = [0, 20000, n]
    X = cfg["xyz"][cut[rank]:cut[rank + 1]]
    P = capi.Problem(*cfg["K"], dtype=capi.EA_F64, device=0)
    P.set_points(X); P.set_dt_grid(cfg["grid"]); P.set_loss(capi.LOSS_CAUCHY, 1.0)
    _set(P)
    out = {}
    q, t, s = P.solve_sharded(Q0, T0, ead.make_allreduce(world))
    out.update(host_q=q, host_t=t, host_it=s["num_iterations"], host_cost=s["final_cost"])
    sums, enqueue = ead.make_device_allreduce(world, torch.device("cuda", 0))
    q, t, s = P.solve_sharded_device(Q0, T0, enqueue, sums.data_ptr(), solve_timeout_ms=20000.0)
    out.update(dev_q=q, dev_t=t, dev_it=s["num_iterations"], dev_cost=s["final_cost"])

    def enqueue_rows(ptr, count, stream):
        ext = torch.cuda.ExternalStream(stream, device=torch.device("cuda", 0))
        with torch.cuda.stream(ext):
            rows = torch.as_tensor(_DeviceDoubles(ptr, count), device=torch.device("cuda", 0))
            h = rows.cpu()
            dist.all_reduce(h, op=dist.ReduceOp.SUM)
            rows.copy_(h)

    def agree(vals):
        tt = torch.tensor(vals, dtype=torch.int32)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        return [int(tt[0]), int(tt[1])]
    q, t, s, used = P.solve_sharded_rows(Q0, T0, enqueue_rows, agree, solve_timeout_ms=20000.0)
    out.update(rows_q=q, rows_t=t, rows_it=s["num_iterations"], rows_cost=s["final_cost"], rows_used=used)
    np.savez(os.path.join(out_dir, "p%d.npz" % rank), **out)
    P.close()
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_prior_counted_once_two_ranks(hip, tmp_path):
    import torch.multiprocessing as mp
    cfg = _problem()
    P = hip.Problem(*cfg["K"], dtype=hip.EA_F64)
    P.set_points(cfg["xyz"]); P.set_dt_grid(cfg["grid"]); P.set_loss(hip.LOSS_CAUCHY, 1.0)
    _set(P, np.sqrt(2.0))
    q2, t2, _ = P.solve(Q0, T0)  # the prior counted twice (H doubled)
    _set(P)
    q, t, s = P.solve(Q0, T0)
    P.close()
    assert max(np.abs(q2 - q).max(), np.abs(t2 - t).max()) > 1e-6
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / "p0.npz"), np.load(tmp_path / "p1.npz")
    assert r0["rows_used"] == 1 and r1["rows_used"] == 1
    for form in ("host", "dev", "rows"):
        assert np.array_equal(r0[form + "_q"], r1[form + "_q"]) and np.array_equal(r0[form + "_t"], r1[form + "_t"]), form
        assert r0[form + "_it"] == r1[form + "_it"] == s["num_iterations"], form
        assert np.abs(r0[form + "_q"] - q).max() < 1e-10 and np.abs(r0[form + "_t"] - t).max() < 1e-10, form
        assert r0[form + "_cost"] == pytest.approx(s["final_cost"], rel=1e-10), form
