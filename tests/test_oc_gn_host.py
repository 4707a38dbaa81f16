"""CPU (no GPU needed): the Gauss-Newton mode's ABI constant and its argument validation at the entry points and in ModelLib.oc_pdp_grad before any launch / foreign call,
the Levenberg-Marquardt loop (pdp_amd.irl.LMLoop, lm_step) on injected evaluations, and parallel.mean_loss_grad_gn without a process group."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_defines_the_flag_beside_the_oc_flags_and_keeps_its_33_entry_points():
    src = open(os.path.join(ROOT, "include", "pdp_hip.h")).read()
    assert re.search(r"^#define\s+PDP_GRAD_GAUSS_NEWTON\s+16\b", src, flags=re.M)
    flags = {k: int(v) for k, v in re.findall(r"^#define\s+(PDP_OC_[A-Z_]+)\s+(\d+)", src, flags=re.M)}
    assert flags == {"PDP_OC_GIVEN_TRAJ": 1, "PDP_OC_PACKED": 2, "PDP_OC_RECORD_PRIMAL": 4, "PDP_OC_COTANGENT": 8}      # no PDP_OC_* define was added; 16 is a new bit
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert len(set(re.findall(r"\b(pdp_[a-z0-9_]+)\s*\(", code))) == 33


def test_entry_points_reject_the_bad_combinations_before_any_launch():
    """Valid (host) pointers everywhere, so that only the flag combination can be what is refused; the horizon is far beyond the kernels' LDS, so that a call that passes
    the argument checks returns PDP_E_SIZE - where it is returned today - and nothing is ever launched, with or without a GPU in the machine."""
    import __graft_entry__ as g
    g.build()
    from pdp_amd import codegen, runtime as rt, zoo
    for system in ("quadrotor", "cartpole"):
        mdl = rt.load_model(codegen.build_problem(zoo.make_problem(system, "irl"))[0])
        B, T = 1, 100000
        keep = [(C.c_double * 8)() for _ in range(16)]
        x0, u, th, dx, du, x, lam, loss, grad, dxdp, dudp, ric, ws = (C.cast(k, C.c_void_p) for k in keep[:13])
        prec, status = C.cast(keep[13], C.c_void_p), C.cast(keep[14], C.c_void_p)
        big = 1 << 60

        def plain(flags, dx_=None, du_=None):
            return mdl.lib.pdp_oc_pdp_grad_batched(B, T, flags, x0, u, th, 0, dx, du, x, lam, loss, grad, dx_, du_, status, ws, big, None)

        def sens(flags, **kw):
            so = rt.PdpOcSensOut(*[kw.get(k).value if k in kw else None for k in ("dxdp", "dudp", "riccati", "predict_record")])
            return mdl.lib.pdp_oc_pdp_grad_sens_batched(B, T, flags, x0, u, th, 0, dx, du, x, lam, loss, grad, C.byref(so), status, ws, big, None)
        assert plain(0) == -2 and plain(16) == -2 and plain(16 | 1) == -2 and sens(16) == -2          # PDP_E_SIZE exactly where it is today
        assert plain(16 | 8) == -1 and plain(16 | 2) == -1 and plain(16 | 8 | 2) == -1 and plain(16 | 2 | 1) == -1
        assert plain(16, dx_=dxdp) == -1 and plain(16, du_=dudp) == -1 and plain(16, dx_=dxdp, du_=dudp) == -1
        assert sens(16, dxdp=dxdp) == -1 and sens(16, dudp=dudp) == -1 and sens(16, riccati=ric) == -1 and sens(16, predict_record=prec) == -1
        assert sens(16 | 8) == -1 and sens(16 | 2) == -1


class _NoForeignCalls:
    def __getattr__(self, name):
        raise AssertionError("foreign call %s before the arguments were validated" % name)


def test_runtime_and_class_surface_reject_the_combinations_before_any_foreign_call():
    from pdp_amd import runtime
    mdl = runtime.ModelLib.__new__(runtime.ModelLib)
    mdl.n, mdl.m, mdl.p, mdl.lib = 4, 1, 7, _NoForeignCalls()
    B, T = 3, 6
    u, th, x0, dx, du = np.zeros((B, T, 1)), np.ones(7), np.zeros((B, 4)), np.zeros((B, T + 1, 4)), np.zeros((B, T, 1))
    for kw in (dict(want_sens=True), dict(want_riccati=True), dict(want_predict_record=True), dict(want_predict_record="primal"), dict(packed=True),
               dict(want_sens=True, want_riccati=True)):
        with pytest.raises(ValueError, match="gauss_newton"):
            mdl.oc_pdp_grad(u, th, dx, du, x0=x0, gauss_newton=True, **kw)
    from pdp_amd import PDP
    oc = PDP.OCSys.__new__(PDP.OCSys)
    for kw in (dict(want_sens=True), dict(want_riccati=True), dict(want_predict_record=True)):
        with pytest.raises(ValueError, match="gauss_newton"):
            oc.pdp_grad_batch(u, th, dx, du, ini_state=x0, want_gauss_newton=True, **kw)


def test_lm_step_is_marquardts_scaled_damping():
    from pdp_amd.irl import lm_step
    G, g = np.array([[4.0, 1.0], [1.0, 9.0]]), np.array([2.0, -3.0])
    assert np.allclose(lm_step(g, G, 0.5), np.linalg.solve(G + 0.5 * np.diag([4.0, 9.0]), g), rtol=1e-15, atol=0)
    # a diagonal entry of 0 is damped by lam itself
    assert np.allclose(lm_step([2.0, 1.0], [[4.0, 0.0], [0.0, 0.0]], 0.5), [2.0 / 6.0, 1.0 / 0.5], rtol=1e-15, atol=0)
    # a damped matrix that is still singular: least squares, not an exception
    s = lm_step([1.0, 1.0], [[1.0, -1.0], [-1.0, 1.0]], 0.0)
    assert np.isfinite(s).all()


def _nlls(theta):
    """three parameters, three residuals; theta[1] - theta[2] moves nothing: J has rank 2 everywhere (one unidentifiable direction), the diagonal of J'J stays positive"""
    a, s = theta[0], theta[1] + theta[2]
    r = np.array([np.exp(a) - 2.0, s - 1.0, s * s - 1.0])
    J = np.array([[np.exp(a), 0.0, 0.0], [0.0, 1.0, 1.0], [0.0, 2 * s, 2 * s]])
    return float(r @ r), J.T @ r, J.T @ J


def test_lm_loop_converges_on_a_rank_deficient_least_squares_problem():
    from pdp_amd.irl import LMLoop
    assert np.linalg.matrix_rank(_nlls(np.array([0.0, 2.0, 1.0]))[2]) == 2
    loop = LMLoop(_nlls, [0.0, 2.0, 1.0])
    r = loop.run(max_evals=40, loss_tol=1e-24)
    assert r["loss_trace"][0] == _nlls(np.array([0.0, 2.0, 1.0]))[0] and r["loss_trace"][-1] <= 1e-24 and not r["stalled"]
    assert (np.diff(r["loss_trace"]) < 0).all() and r["evaluations"] == len(r["loss_trace"]) + r["rejected"] <= 40
    th = r["parameter_trace"][-1]
    assert abs(th[0] - np.log(2.0)) <= 1e-12 and abs(th[1] + th[2] - 1.0) <= 1e-12
    assert abs((th[1] - th[2]) - 1.0) <= 1e-9               # the unidentifiable direction is left where it started (the damped step is orthogonal to it)
    assert r["parameter_trace"].shape == (len(r["loss_trace"]), 3) and r["lambda_trace"].shape == r["loss_trace"].shape and r["iterations"] == len(r["loss_trace"])


def test_lm_loop_accept_reject_lambda_sequence_equals_the_hand_written_one():
    """r(theta) = theta (p = 1): loss theta^2, g = theta, G = 1, so the trial from theta at damping lam is theta lam / (1 + lam).  The second evaluation is declared
    not evaluable (None), the sixth returns a loss that is not below the current one."""
    from pdp_amd.irl import LMLoop
    calls = []

    def evaluate(theta):
        calls.append(float(theta[0]))
        if len(calls) == 2:
            return None
        if len(calls) == 6:
            return calls[-2] ** 2, theta, np.ones((1, 1))        # equal, not strictly below: rejected
        return float(theta[0] ** 2), theta.copy(), np.ones((1, 1))
    loop = LMLoop(evaluate, [1.0], lam0=1.0, up=10.0, down=10.0)
    loop.start()
    assert (loop.lam, loop.evaluations, loop.rejected) == (1.0, 1, 0)
    seq = [(loop.step(), loop.lam) for _ in range(6)]
    #        trial 1/2: None      10/11 from lam 10    (10/11)/2 from 1    x 0.1/1.1 from 0.1    equal loss           again from lam 0.1
    assert [a for a, _ in seq] == [False, True, True, True, False, True]
    assert np.allclose([l for _, l in seq], [10.0, 1.0, 0.1, 0.01, 0.1, 0.01], rtol=1e-14, atol=0)
    t3 = 10.0 / 11.0 / 2.0 * (0.1 / 1.1)
    assert np.allclose(calls, [1.0, 0.5, 10.0 / 11.0, 10.0 / 22.0, t3, t3 * 0.01 / 1.01, t3 * 0.1 / 1.1], rtol=1e-12, atol=0)
    r = loop.results()
    assert (r["evaluations"], r["rejected"], r["stalled"]) == (7, 2, False)
    assert np.allclose(r["loss_trace"], np.array([1.0, 10.0 / 11.0, 10.0 / 22.0, t3, t3 * 0.1 / 1.1]) ** 2, rtol=1e-12, atol=0)
    assert np.allclose(r["lambda_trace"], [1.0, 1.0, 0.1, 0.01, 0.01], rtol=1e-14, atol=0)
    assert np.allclose(r["parameter_trace"][:, 0], [1.0, 10.0 / 11.0, 10.0 / 22.0, t3, t3 * 0.1 / 1.1], rtol=1e-12, atol=0)


def test_lm_loop_stalls_cleanly_at_lam_max_and_respects_lam_min_and_max_evals():
    from pdp_amd.irl import LMLoop
    flat = lambda theta: (1.0, np.ones(1), np.ones((1, 1)))        # no trial ever improves
    loop = LMLoop(flat, [0.0], lam0=1.0, up=10.0, lam_max=1e3)
    r = loop.run(max_evals=100)
    assert r["stalled"] and (r["evaluations"], r["rejected"]) == (5, 4) and loop.lam == 1e4 and list(r["loss_trace"]) == [1.0]
    loop = LMLoop(flat, [0.0], lam0=1.0, up=10.0, lam_max=1e3)
    r = loop.run(max_evals=3)
    assert not r["stalled"] and r["evaluations"] == 3
    lin = lambda theta: (float(theta[0] ** 2), theta.copy(), np.ones((1, 1)))
    loop = LMLoop(lin, [1.0], lam0=1e-11, lam_min=1e-12)
    loop.run(max_evals=4, loss_tol=0.0)
    assert loop.lam == 1e-12
    with pytest.raises(RuntimeError, match="initial parameter"):
        LMLoop(lambda theta: None, [1.0]).run()


def test_mean_loss_grad_gn_splits_a_row_without_a_process_group():
    import torch
    from pdp_amd import parallel
    p, B = 3, 4
    rng = np.random.default_rng(0)
    rows = torch.as_tensor(rng.standard_normal((B, p + 1 + p * p)))
    loss, g, G = parallel.mean_loss_grad_gn(rows, p)
    m = rows.numpy().mean(axis=0)
    assert g.shape == (p,) and G.shape == (p, p) and loss.dim() == 0
    assert np.allclose(g.numpy(), m[:p], rtol=1e-15) and np.allclose(float(loss), m[p], rtol=1e-15) and np.allclose(G.numpy(), m[p + 1:].reshape(p, p), rtol=1e-15)
    loss2, _, G2 = parallel.mean_loss_grad_gn(rows, p, n_total=2 * B)      # this rank's share of a larger batch
    assert np.allclose(float(loss2), m[p] / 2, rtol=1e-15) and np.allclose(G2.numpy(), m[p + 1:].reshape(p, p) / 2, rtol=1e-15)
    with pytest.raises(ValueError, match="p \\+ 1 \\+ p p"):
        parallel.mean_loss_grad_gn(rows[:, :-1], p)


# ---- two ranks over gloo: the accept / reject decision of a sharded Levenberg-Marquardt loop is collective --------------------------------------------------------------
_A = np.array([1.0, -0.5, 2.0, 0.7, -1.3])          # five samples (ragged over two ranks: 3 + 2), residual r_i = a_i exp(theta_0) + b_i theta_1 - y_i
_Bc = np.array([0.3, 1.1, -0.8, 0.5, 2.0])
_Y = _A * np.exp(0.4) + _Bc * (-1.5)                # zero residual at theta = (0.4, -1.5)
_FAIL_AT = (2, 4)                                   # evaluations in which ONE rank (rank 1; the lone process in the reference run) finds a sample it cannot use


def _sharded_rows(theta, idx):
    import torch
    e = np.exp(theta[0])
    r = _A[idx] * e + _Bc[idx] * theta[1] - _Y[idx]
    J = np.stack([_A[idx] * e, _Bc[idx]], axis=1)                                  # [b, 2]
    rows = np.concatenate([J * r[:, None], (r * r)[:, None], (J[:, :, None] * J[:, None, :]).reshape(len(idx), 4)], axis=1)      # gradient | loss | G
    return torch.as_tensor(rows)


def _run_sharded_lm(idx, failing, n_total):
    import torch
    from pdp_amd import parallel
    from pdp_amd.irl import LMLoop
    calls = [0]

    def evaluate(theta):
        calls[0] += 1
        bad = torch.tensor([1.0 if (failing and calls[0] in _FAIL_AT) else 0.0], dtype=torch.float64)
        row = parallel.mean_row_checked(_sharded_rows(theta, idx), bad, n_total)    # EVERY rank gets here in EVERY evaluation: the flag travels with the rows
        return None if row is None else (float(row[2]), row[:2].copy(), row[3:].reshape(2, 2).copy())
    loop = LMLoop(evaluate, [0.0, 0.0])
    r = loop.run(max_evals=25, loss_tol=1e-26)
    return r, calls[0]


def _lm_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from pdp_amd import parallel
    lo, hi = parallel.shard_bounds(5, world, rank)
    r, ncalls = _run_sharded_lm(np.arange(lo, hi), failing=(rank == 1), n_total=None if rank == 0 else 5)      # (the count exchanged, and given)
    dist.barrier()                                                                  # every collective of the run was matched: nobody is left waiting
    q.put((rank, r["loss_trace"], r["parameter_trace"], r["lambda_trace"], r["evaluations"], r["rejected"], r["stalled"], ncalls, hi - lo))
    dist.destroy_process_group()


def test_two_ranks_reject_a_trial_together_when_one_of_them_cannot_evaluate_it():
    """A rank that returned None on its own flags before the exchange would skip a collective the other rank issues: the ranks would pair all-reduces of different trials,
    drift apart and end on an unmatched collective.  Here rank 1 alone finds a bad sample in evaluations 2 and 4; both ranks must reject exactly those trials, keep
    identical traces and dampings, and equal the single-process run with the same failures."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_lm_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    ref, ncalls = _run_sharded_lm(np.arange(5), failing=True, n_total=5)
    assert ref["rejected"] >= 2 and ref["loss_trace"][-1] <= 1e-26 and not ref["stalled"] and ncalls == ref["evaluations"]
    assert sorted(t[8] for t in res) == [2, 3]
    a, b = res
    for k in (1, 2, 3):                                                            # the same message on both ranks: identical to the bit
        assert np.array_equal(a[k], b[k])
    assert a[4:8] == b[4:8] == (ref["evaluations"], ref["rejected"], False, ncalls)
    assert np.array_equal(a[3], ref["lambda_trace"])                               # the same accept / reject sequence as one process
    # the sharded sum differs from the single sum by rounding: ~1e-15 absolute in a residual, so ~1e-15 / sqrt(loss) relative in a loss - compared where that is <= 1e-9
    big = ref["loss_trace"] >= 1e-12
    assert big.sum() >= 4 and np.allclose(a[1][big], ref["loss_trace"][big], rtol=1e-8, atol=0) and a[1][-1] <= 1e-26
    assert np.allclose(a[2], ref["parameter_trace"], rtol=1e-12, atol=0)
    assert np.allclose(a[2][-1], [0.4, -1.5], rtol=1e-10, atol=0)
