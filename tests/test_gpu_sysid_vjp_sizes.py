"""GPU: sysid_vjp_kernel (pdp_sysid_rollout_vjp_batched) where a user's model differs from the zoo - pools of 4, 8 and 16 rows cut into several chunks, one to four
64-lane parameter slots (full, barely started, partial), n = 64 (every lane owns a costate), instantiations that spill registers, and the large-batch row clamp where it
changes the chunking.  Models: tests/sysid_vjp_common.py SIZE_MODELS, built once with hipcc and cached by content hash.  Reference: forward sensitivities through
SysIDOracle from sympy (sv.reference), bound sv.TOL = 1e-10 of the largest entry per sample; B = 3, inputs and cotangents N(0,1)."""
import numpy as np
import pytest

import sysid_vjp_common as sv

pytestmark = pytest.mark.gpu
TOL = sv.TOL
_infos = {}


def npy(t):
    return t.detach().cpu().numpy()


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def model(name):
    return sv.user_pair(name)[0].model()


def generated_chunk(name):
    from pdp_amd import codegen
    if name not in _infos:
        _infos[name] = codegen.generate(sv.size_problem(name)[0])[1]
    return _infos[name]["chunk"]


def run(mdl, c, g=None, **kw):
    """rollout on the GPU from the case's initial states, then the entry point: (states, dict of numpy outputs)"""
    x = mdl.sysid_integrate(c["x0"], c["inputs"], c["theta"])
    out = mdl.sysid_rollout_vjp(x, c["inputs"], c["theta"], c["g"] if g is None else g, **kw)
    return x, {k: npy(v) for k, v in out.items()}


def check_case(margins, tag, mdl, c):
    """rollout, grad_theta and grad_x0 within TOL of the case's reference; each output alone (the other pointer NULL) has the joint launch's bits"""
    x, out = run(mdl, c)
    margins.check(tag + ": rollout", sv.rel_rows(npy(x), c["states"]), TOL)
    margins.check(tag + ": grad_theta", sv.rel_rows(out["grad_theta"], c["grad_theta"]), TOL)
    margins.check(tag + ": grad_x0", sv.rel_rows(out["grad_x0"], c["grad_x0"]), TOL)
    _, only_theta = run(mdl, c, want_ini=False)
    _, only_ini = run(mdl, c, want_theta=False)
    assert set(only_theta) == {"grad_theta"} and set(only_ini) == {"grad_x0"}
    assert same_bits(only_theta["grad_theta"], out["grad_theta"]) and same_bits(only_ini["grad_x0"], out["grad_x0"]), tag
    return x, out


def check_single_step(margins, tag, c, x, out):
    """T = 1: grad_theta = E_0' g_1, grad_x0 = g_0 + F_0' g_1 from the oracle's Jacobians directly"""
    for b in range(len(c["x0"])):
        th = c["theta"][b] if np.ndim(c["theta"]) == 2 else c["theta"]
        aux = c["orc"].getAuxSys(npy(x)[b], c["inputs"][b], th)
        margins.check("%s sample %d: E_0' g_1" % (tag, b), sv.rel_rows(out["grad_theta"][b:b + 1], (aux["dynE"][0].T @ c["g"][b, 1])[None]), TOL)
        margins.check("%s sample %d: g_0 + F_0' g_1" % (tag, b), sv.rel_rows(out["grad_x0"][b:b + 1], (c["g"][b, 0] + aux["dynF"][0].T @ c["g"][b, 1])[None]), TOL)


def test_chunk_edges_with_four_rows_and_four_parameter_slots(margins):
    """mlp_6_2_246 (p = 246: four slots, 54 live lanes in the last; a pool of R = 4 rows; a kernel that spills): T = 1, R - 1, R, R + 1, 2 R + 1, 3 R + 1 - one to four
    chunks of equal length - with a shared and a per-sample theta; shorter horizons are prefixes of the longest with their own reference"""
    name = "mlp_6_2_246"
    mdl = model(name)
    R = mdl.sysid_vjp_rows(3, cus())
    assert R == mdl.chunk == 4 and (mdl.n, mdl.m, mdl.p) == (6, 2, 246) and (mdl.p + 63) // 64 == 4 and mdl.p - 3 * 64 == 54
    long = sv.user_case(name, T=3 * R + 1)
    for T in (1, R - 1, R, R + 1, 2 * R + 1, 3 * R + 1):
        for key in ("theta", "theta_b"):
            c = sv.prefix(long, T, key)
            tag = "sysid vjp %s T = %d %s theta" % (name, T, "per-sample" if key == "theta_b" else "shared")
            x, out = check_case(margins, tag, mdl, c)
            if T == 1:
                check_single_step(margins, tag, c, x, out)


def test_sixty_four_states(margins):
    """chain_64_4_3 (n = 64: every lane owns a costate, the broadcast reads lanes 0 .. 63; R = 8; a kernel that spills): T = 1, R, R + 1, 2 R + 1; at the longest a
    cotangent in component 63 of x_T alone and one in component 0 alone; zero cotangents give exact zeros"""
    name = "chain_64_4_3"
    mdl = model(name)
    R = mdl.sysid_vjp_rows(3, cus())
    assert R == mdl.chunk == 8 and (mdl.n, mdl.m, mdl.p) == (64, 4, 3)
    long = sv.user_case(name, T=2 * R + 1)
    for T in (1, R, R + 1, 2 * R + 1):
        c = sv.prefix(long, T)
        tag = "sysid vjp %s T = %d" % (name, T)
        x, out = check_case(margins, tag, mdl, c)
        if T == 1:
            check_single_step(margins, tag, c, x, out)
    z = np.zeros_like(long["g"])
    _, out = run(mdl, long, g=z)
    assert not out["grad_theta"].any() and not out["grad_x0"].any()
    for comp in (63, 0):
        g = z.copy()
        g[:, -1, comp] = long["g"][:, -1, comp]
        _, gt, g0 = sv.reference(long["orc"], long["x0"], long["inputs"], long["theta"], g)
        assert np.abs(gt).max(axis=1).min() > 0 and np.abs(g0).max(axis=1).min() > 0
        _, out = run(mdl, long, g=g)
        margins.check("sysid vjp %s T = %d, cotangent in component %d of x_T only: grad_theta" % (name, 2 * R + 1, comp), sv.rel_rows(out["grad_theta"], gt), TOL)
        margins.check("sysid vjp %s T = %d, cotangent in component %d of x_T only: grad_x0" % (name, 2 * R + 1, comp), sv.rel_rows(out["grad_x0"], g0), TOL)


@pytest.mark.parametrize("name", ["linear_8_1_64", "linear_8_1_65"])
def test_parameter_slot_edges(margins, name):
    """p = 64 (one slot, every lane live) and p = 65 (a second slot with one live lane) at T = R + 1; the 65th parameter's gradient on its own, relative to itself;
    and, through the raw entry point into buffers with a NaN row in front and behind, nothing is written outside [B, p] and [B, n]"""
    import torch
    from pdp_amd import runtime as rt
    mdl = model(name)
    R = mdl.sysid_vjp_rows(3, cus())
    assert R == mdl.chunk == generated_chunk(name) and mdl.p == int(name[-2:]) and mdl.n == 8
    c = sv.user_case(name, T=R + 1)
    tag = "sysid vjp %s T = %d" % (name, R + 1)
    x, out = check_case(margins, tag, mdl, c)
    if mdl.p == 65:
        got, want = out["grad_theta"][:, 64], c["grad_theta"][:, 64]
        margins.check(tag + ": grad_theta[:, 64] relative to itself", float((np.abs(got - want) / np.abs(want)).max()), TOL)
    B, T = c["inputs"].shape[:2]
    gt = torch.full((B + 2, mdl.p), float("nan"), dtype=torch.float64, device="cuda")
    g0 = torch.full((B + 2, mdl.n), float("nan"), dtype=torch.float64, device="cuda")
    u, th, g = rt.dev(c["inputs"]), rt.dev(c["theta"]), rt.dev(c["g"])
    rt.check(mdl.lib.pdp_sysid_rollout_vjp_batched(B, T, rt.ptr(x), rt.ptr(u), rt.ptr(th), 0, rt.ptr(g), rt.ptr(gt[1:]), rt.ptr(g0[1:]), rt.current_stream_ptr()),
             "pdp_sysid_rollout_vjp_batched")
    gt, g0 = npy(gt), npy(g0)
    assert same_bits(gt[1:B + 1], out["grad_theta"]) and same_bits(g0[1:B + 1], out["grad_x0"])
    assert np.isnan(gt[0]).all() and np.isnan(gt[B + 1]).all() and np.isnan(g0[0]).all() and np.isnan(g0[B + 1]).all()


def test_the_row_clamp_changes_the_chunks_and_no_bit(margins):
    """linear_9_2_99 (row stride 189): 16 pool rows up to four trajectories per CU, 2400 / 189 = 12 beyond.  T = 13 is one chunk in the small batch and two (7 + 6) in the
    large one, T = 25 is 13 + 12 against 9 + 9 + 7.  Three trajectories sent alone (B = 1) and at the first, middle and last position of B = 4 #CU + 1: the same bits,
    and within TOL of the reference"""
    import torch
    name = "linear_9_2_99"
    mdl = model(name)
    B = 4 * cus() + 1
    assert mdl.sysid_vjp_rows(3, cus()) == 16 and mdl.sysid_vjp_rows(1, cus()) == 16 and mdl.sysid_vjp_rows(B, cus()) == 12
    long = sv.user_case(name, T=25)
    for T in (13, 25):
        c = sv.prefix(long, T)
        alone = [run(mdl, dict(x0=c["x0"][b:b + 1], inputs=c["inputs"][b:b + 1], theta=c["theta"], g=c["g"][b:b + 1]))[1] for b in range(3)]
        pos = [0, B // 2, B - 1]
        idx = np.arange(B) % 3
        idx[pos] = [0, 1, 2]
        _, out = run(mdl, dict(x0=c["x0"][idx], inputs=c["inputs"][idx], theta=c["theta"], g=c["g"][idx]))
        for k, b in enumerate(pos):
            assert same_bits(out["grad_theta"][b], alone[k]["grad_theta"][0]) and same_bits(out["grad_x0"][b], alone[k]["grad_x0"][0]), (T, b)
        margins.check("sysid vjp %s T = %d, B = %d (12 pool rows): grad_theta" % (name, T, B), sv.rel_rows(out["grad_theta"][pos], c["grad_theta"]), TOL)
        margins.check("sysid vjp %s T = %d, B = %d (12 pool rows): grad_x0" % (name, T, B), sv.rel_rows(out["grad_x0"][pos], c["grad_x0"]), TOL)
        margins.check("sysid vjp %s T = %d, B = 1 (16 pool rows): grad_theta" % (name, T), sv.rel_rows(np.concatenate([a["grad_theta"] for a in alone]), c["grad_theta"]), TOL)
        margins.check("sysid vjp %s T = %d, B = 1 (16 pool rows): grad_x0" % (name, T), sv.rel_rows(np.concatenate([a["grad_x0"] for a in alone]), c["grad_x0"]), TOL)
    torch.cuda.synchronize()


def test_the_layer_with_four_parameter_slots(margins):
    """sysid_trajectory on mlp_6_2_246, B = 3, T = 5, L = sum w . state^2: a [B, p] theta gets the per-sample rows, a shared [p] theta their sum over the batch, and
    ini_state.grad is the reference's grad_x0"""
    import torch
    from pdp_amd.autograd import sysid_trajectory
    name = "mlp_6_2_246"
    c = sv.user_case(name, T=13)
    sid, orc = c["sid"], c["orc"]
    B, T = 3, 5
    x0, inputs, w = c["x0"], c["inputs"][:, :T], np.abs(c["g"][:, :T + 1])
    wd, ud = torch.as_tensor(w, device="cuda"), torch.as_tensor(inputs, device="cuda")
    for key in ("theta_b", "theta"):
        theta = torch.tensor(c[key], device="cuda", dtype=torch.float64, requires_grad=True)
        ini = torch.tensor(x0, device="cuda", dtype=torch.float64, requires_grad=True)
        state = sysid_trajectory(sid, ini, ud, theta)
        assert tuple(state.shape) == (B, T + 1, 6)
        (wd * state ** 2).sum().backward()
        xs, _, _ = sv.reference(orc, x0, inputs, c[key], np.zeros((B, T + 1, 6)))
        _, gt, g0 = sv.reference(orc, x0, inputs, c[key], 2.0 * w * xs)
        want = gt if key == "theta_b" else gt.sum(axis=0)[None]
        assert tuple(theta.grad.shape) == tuple(c[key].shape)
        margins.check("sysid layer, %s, %s: theta.grad" % (name, key), sv.rel_rows(npy(theta.grad).reshape(want.shape), want), TOL)
        margins.check("sysid layer, %s, %s: ini_state.grad" % (name, key), sv.rel_rows(npy(ini.grad), g0), TOL)


def test_a_nan_stays_in_its_trajectory_when_registers_spill():
    """mlp_6_2_246, T = 2 R + 1, NaN in g[1, R + 1, 2]: samples 0 and 2 keep the clean run's bits, sample 1 is NaN in both outputs"""
    name = "mlp_6_2_246"
    mdl = model(name)
    R = mdl.chunk
    c = sv.prefix(sv.user_case(name, T=3 * R + 1), 2 * R + 1)
    _, clean = run(mdl, c)
    assert np.isfinite(clean["grad_theta"]).all() and np.isfinite(clean["grad_x0"]).all()
    g = c["g"].copy()
    g[1, R + 1, 2] = np.nan
    _, out = run(mdl, c, g=g)
    assert np.isnan(out["grad_x0"][1]).any() and np.isnan(out["grad_theta"][1]).any()
    for b in (0, 2):
        assert same_bits(out["grad_theta"][b], clean["grad_theta"][b]) and same_bits(out["grad_x0"][b], clean["grad_x0"][b])
