"""GPU: the ControlPlanning.step kernels on user models at their tile edges - the three models of tests/cp_edge_common.py (C16: n = 16, m = 4, no padding row in any
state tile, a network's first layer fills all 16 lanes; C15: n = 15, m = 3; C5: n = 5, m = 1) under the Lagrange policy (1 - 4 sensitivity tiles of 16 parameters, a
partial last tile, a pivot straddling two tiles, horizons of one step, one full chunk, two unequal chunks, three chunks) and tanh networks (one to four layers, width
16, non-square hidden layers on the register kernels; widths 17 - 32 and eight layers on the adjoint kernel; p > 512, width 33 and nine layers handed to the
size-generic kernel), every sample against oracle.pdp_oracle.ControlPlanningOracle on the same inputs.

The kernel-selecting variables are read once per process, so each environment runs in one child process that evaluates every applicable case and saves an .npz:
    default    switches unset: what a user gets at B = 5 (one-wave Lagrange kernel with the tiles over grid.y, one-trajectory register kernel, adjoint kernel, generic kernel)
    one_wave   PDP_CP_POLY_VARIANT=1 PDP_CP_PREPASS=0 PDP_CP_MLP_VARIANT=1: cp_step_poly_kernel<NT> (NT = 1 at B = 5, NT = all tiles at B = 2 CUs + 1), cp_step_adjoint_kernel
               (resident at B = 5, activations offloaded at the batch of cp_edge_common.offload_batch)
    pair       PDP_CP_POLY_VARIANT=3 PDP_CP_PREPASS=0 PDP_CP_MLP_VARIANT=3: cp_step_poly2_kernel<NT, 1> (<NT, 2> and <NT, 4> at B = CUs + 1 and 2 CUs + 1), cp_step_mlp16_kernel
    four       PDP_CP_MLP_VARIANT=4: cp_step_mlp4t_kernel<NL> for the shared theta (B = 5 leaves the second wavefront ragged), cp_step_mlp16_kernel for per-sample theta
    given      PDP_CP_PREPASS=1: cp_poly_rollout_lanes_kernel + cp_step_poly_kernel<NT, true>
tests/test_cp_edge_inputs.py holds what makes this mean something: the restated routing rules send every case to the kernel named here, and the oracle's own rounding
error is below 1e-13 of every parameter block on these inputs.

Tolerances (tests/test_gpu_generic_sizes.py): loss 1e-11 relative; state and control trajectories 1e-10 of their largest entry; gradient 1e-10 of
the largest entry OF EACH BLOCK (cp_edge_common.blocks: the 16-column tiles, each vec(A_k) and each b_k), per sample, through the `margins` fixture - one line per
(environment, model, policy family, quantity) with the largest figure over cases, horizons, theta modes and samples.  A call without trajectory outputs returns the loss
and gradient of the call with them, bit for bit.

The three model libraries are compiled on first use (`built` compiles them side by side; host time)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import cp_edge_common as c  # noqa: E402

NAMES = c.NAMES
ENV = {"default": {},
       "one_wave": dict(PDP_CP_POLY_VARIANT="1", PDP_CP_PREPASS="0", PDP_CP_MLP_VARIANT="1"),
       "pair": dict(PDP_CP_POLY_VARIANT="3", PDP_CP_PREPASS="0", PDP_CP_MLP_VARIANT="3"),
       "four": dict(PDP_CP_MLP_VARIANT="4"),
       "given": dict(PDP_CP_PREPASS="1")}
SWITCHES = ("PDP_CP_POLY_VARIANT", "PDP_CP_PREPASS", "PDP_CP_MLP_VARIANT", "PDP_CP_GIVEN_WGS", "PDP_CP_MLP_LDS_KB", "PDP_CP_GENERIC_WIDE_BYTES")
POLY_TAGS = ("default", "one_wave", "pair", "given")
MLP_TAGS = ("default", "one_wave", "pair", "four")
BIG_TAGS = ("pair", "one_wave", "given")
MLP_ROUTES = {"default": ("register", "adjoint"), "one_wave": ("register", "adjoint"), "pair": ("register",), "four": ("register",)}     # (the hand-over cases: default alone)
KERNELS = {("default", "poly"): "cp_step_poly_kernel<1>, tiles over grid.y", ("one_wave", "poly"): "cp_step_poly_kernel<1>, tiles over grid.y",
           ("pair", "poly"): "cp_step_poly2_kernel<1, 1>, tiles over grid.y", ("given", "poly"): "cp_poly_rollout_lanes_kernel + cp_step_poly_kernel<NT, true>",
           ("default", "mlp"): "cp_step_mlp16_kernel / cp_step_adjoint_kernel", ("one_wave", "mlp"): "cp_step_adjoint_kernel", ("pair", "mlp"): "cp_step_mlp16_kernel",
           ("four", "mlp"): "cp_step_mlp4t_kernel<NL> (shared theta) / cp_step_mlp16_kernel (per-sample theta)"}
FILL = 7.0
PDP_E_ARG = -1


def npy(t):
    return t.detach().cpu().numpy()


def _key(kind, name, key, T, per_sample=None):
    ks = "x".join(map(str, key)) if kind == "mlp" else str(key)
    return "%s|%s|%s|%d|" % (kind, name, ks, T) + ("" if per_sample is None else "%d|" % per_sample)


# ---- child process ------------------------------------------------------------------------------------------------------------------------------------------
def _policy(kind, key, T):
    from pdp_amd import runtime as rt
    return rt.make_policy("poly", pivots=np.linspace(0, T, key)) if kind == "poly" else rt.make_policy("mlp", layers=list(key))


def _step(out, mdl, name, kind, key, T):
    """one case, shared and per-sample theta: the call with trajectory outputs, and whether the call without them returns the same bits"""
    import torch
    inp = c.inputs(name, kind, key, T)
    pol = _policy(kind, key, T)
    for per_sample in (0, 1):
        th = inp["theta_b"] if per_sample else inp["theta"]
        loss, grad, x, u = mdl.cp_step(pol, inp["p"], inp["x0"], th, T, want_traj=True)
        l2, g2 = mdl.cp_step(pol, inp["p"], inp["x0"], th, T)
        k = _key(kind, name, key, T, per_sample)
        out[k + "loss"], out[k + "grad"], out[k + "x"], out[k + "u"] = npy(loss), npy(grad), npy(x), npy(u)
        out[k + "same"] = np.array([bool(torch.equal(loss, l2)), bool(torch.equal(grad, g2))])


def _big(out, mdl, name, kind, key, T, B, label, rows):
    """a large batch (shared theta): the listed rows of every output, and the whole loss and gradient"""
    inp = c.inputs(name, kind, key, T)
    x0 = c.big_rows(name, kind, key, T, B)
    loss, grad, x, u = mdl.cp_step(_policy(kind, key, T), inp["p"], x0, inp["theta"], T, want_traj=True)
    k = "big|%s|%s|" % (label, name)
    out[k + "B"], out[k + "rows"] = np.array(B), np.array(rows)
    out[k + "loss"], out[k + "grad"], out[k + "x"], out[k + "u"] = npy(loss), npy(grad), npy(x[rows]), npy(u[rows])


def _argument_errors(out, mdl, name):
    """N = 17 pivots, and a parameter count that does not match the policy: PDP_E_ARG, and nothing is written (outputs filled with 7.0 beforehand)"""
    import ctypes as C
    import torch
    from pdp_amd import runtime as rt
    n, m = c.MODELS[name]
    T, B = 7, c.B_UNIT
    x0 = rt.dev(c.inputs(name, "poly", 6, T)["x0"])
    pol17 = rt.make_policy("poly", pivots=np.linspace(0, T, 16))
    pol17.n_pivots = 17
    net = c.CLASS_MLP[name]
    calls = {"pivots17": (pol17, 17 * m), "poly_p_plus_1": (_policy("poly", 6, T), 6 * m + 1), "poly_p_minus_1": (_policy("poly", 6, T), 6 * m - 1),
             "mlp_p_plus_1": (_policy("mlp", net, T), c.mlp_params(n, net) + 1)}
    for label, (pol, p) in calls.items():
        th = torch.full((p + 8,), 0.1, dtype=torch.float64, device="cuda")
        outs = [torch.full(s, FILL, dtype=torch.float64, device="cuda") for s in ((B,), (B, p + 8), (B, T + 1, n), (B, T, m))]
        ws = torch.full((1 << 20,), FILL, dtype=torch.float64, device="cuda")
        rc = mdl.lib.pdp_cp_step_batched(B, T, C.byref(pol), p, rt.ptr(x0), rt.ptr(th), 0, rt.ptr(outs[0]), rt.ptr(outs[1]), rt.ptr(outs[2]), rt.ptr(outs[3]), rt.ptr(ws),
                                         ws.numel() * 8, rt.current_stream_ptr())
        torch.cuda.synchronize()
        out["err|%s|%s" % (name, label)] = np.array([rc] + [int(bool((t == FILL).all())) for t in outs + [ws]])


def _class_surface(out, name, cp):
    """ControlPlanning.integrateSys_batch / getAuxSys_batch / step_batch: cp_integrate_kernel and cp_auxsys_kernel (lane-local arrays sized by the policy description)"""
    T = c.CLASS_T
    for kind, key in (("poly", 6), ("mlp", c.CLASS_MLP[name])):
        inp = c.inputs(name, kind, key, T)
        if kind == "poly":
            cp.setPolyControl(np.linspace(0, T, key))
        else:
            cp.setNeuralPolicy(list(key[:-1]))
        assert cp.n_auxvar == inp["p"]
        for per_sample in (0, 1):
            th = inp["theta_b"] if per_sample else inp["theta"]
            x, u, cost = cp.integrateSys_batch(inp["x0"], T, th)
            aux = cp.getAuxSys_batch(x, u, th)
            loss, grad = cp.step_batch(inp["x0"], T, th)
            k = "class|" + _key(kind, name, key, T, per_sample)
            for lab, v in (("x", x), ("u", u), ("cost", cost), ("loss", loss), ("grad", grad), ("dynF", aux["dynF"]), ("dynG", aux["dynG"]), ("dUx", aux["dUx"]), ("dUe", aux["dUe"])):
                out[k + lab] = npy(v)


def _worker(tag):
    """runs in a child process whose environment selects the kernels; every entry point returned 0 (runtime.check raises otherwise)"""
    import ctypes as C
    import torch
    out = {}
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out["cus"] = np.array(cus)
    cps = {name: c.model_gpu(name) for name in NAMES}
    for name in NAMES:
        mdl = cps[name].model()             # compiled by now (the `built` fixture), else on this first use
        assert (mdl.n, mdl.m, mdl.chunk) == c.MODELS[name] + (c.CHUNK,)
    for name in NAMES:
        mdl = cps[name].model()
        if tag in POLY_TAGS:
            for _, N, T in c.poly_cases(name):
                _step(out, mdl, name, "poly", N, T)
            _argument_errors(out, mdl, name)
        if tag in MLP_TAGS:
            for _, layers, T in c.mlp_cases(name, MLP_ROUTES[tag] + (("generic",) if tag == "default" else ())):
                _step(out, mdl, name, "mlp", layers, T)
        if tag == "given":                  # the workspace the host asks for is the pre-pass's: x | u | h_x per trajectory
            for _, N, T in c.poly_cases(name):
                out["ws|" + _key("poly", name, N, T)] = np.array(mdl.lib.pdp_cp_step_workspace_bytes(c.B_UNIT, T, C.byref(_policy("poly", N, T)), N * mdl.m))
        if tag in BIG_TAGS:                 # the workgroup shapes of the pair kernel (two and four trajectories per workgroup, a ragged last one); the one-wave kernel with
            for B in (cus + 1, 2 * cus + 1):    # all tiles in one workgroup and the lane-per-trajectory pre-pass over several workgroups (a ragged last one), on the same batches
                _big(out, mdl, name, "poly", c.PAIR_PIVOTS[name], c.PAIR_T, B, "B%d" % (B // cus), [0, B // 2, B - 1])
        if tag == "default":
            _class_surface(out, name, cps[name])
        print("%s %s done" % (tag, name), flush=True)
    if tag == "one_wave":                   # the adjoint kernel with its activations in the workspace
        name, layers, T = c.OFFLOAD_CASE
        B = c.offload_batch(cus)
        assert B > 0
        out["offload_ws"] = np.array(cps[name].model().lib.pdp_cp_step_workspace_bytes(B, T, C.byref(_policy("mlp", layers, T)), c.mlp_params(c.MODELS[name][0], layers)))
        _big(out, cps[name].model(), name, "mlp", layers, T, B, "offload", [0, 1, 2, 3, 4, B // 2, B - 1])
    return out


# ---- parent -------------------------------------------------------------------------------------------------------------------------------------------------
_results, _stopped = {}, []


@pytest.fixture(scope="module")
def built():
    """the three model libraries, compiled side by side where they are not there yet (content-hash cache of codegen.build_problem)"""
    import time
    from concurrent.futures import ThreadPoolExecutor
    from pdp_amd import codegen

    def build(name):
        t = time.time()
        lib = codegen.build_problem(c.problem(name))[0]
        return lib, time.time() - t
    with ThreadPoolExecutor(max_workers=3) as ex:
        res = dict(zip(NAMES, ex.map(build, NAMES)))
    print("model libraries (seconds; near zero when cached): " + ", ".join("%s %.1f" % (k, v[1]) for k, v in res.items()))
    return {k: v[0] for k, v in res.items()}


@pytest.fixture(scope="module")
def run(built, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cp_edge")

    def _run(tag):
        if tag not in _results:
            # a child that died (a fault, a time limit) ends the GPU work of this module: nothing more is started on the device
            assert not _stopped, "not started: the child process of environment %r failed before" % _stopped[0]
            f = os.path.join(str(tmp), tag + ".npz")
            code = "import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_cp_edge as m; np.savez(%r, **m._worker(%r))" % (ROOT, HERE, f, tag)
            env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
            try:
                r = subprocess.run([sys.executable, "-c", code], env=dict(env, **ENV[tag]), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
            except subprocess.TimeoutExpired:
                _stopped.append(tag)
                raise
            if r.returncode != 0:
                _stopped.append(tag)
            assert r.returncode == 0, "environment %s: exit %d\n%s" % (tag, r.returncode, r.stdout[-4000:])
            _results[tag] = dict(np.load(f))
        return _results[tag]
    return _run


class _Worst:
    """the largest figure per quantity, and where it occurred"""

    def __init__(self):
        self.v = {}

    def add(self, quantity, value, where):
        prev = self.v.get(quantity)
        if prev is None or (prev[0] == prev[0] and not (value <= prev[0])):      # (a NaN comes in and stays)
            self.v[quantity] = (float(value), where)

    def check(self, margins, tag, bounds):
        for quantity, (value, where) in self.v.items():
            print("%s: %s %.3e at %s" % (tag, quantity, value, where))
        for quantity, (value, where) in self.v.items():
            margins.check("cp edge %s: %s" % (tag, quantity), value, bounds[quantity])


BOUNDS = {"loss (relative)": c.TOL_LOSS, "state trajectory": c.TOL, "control trajectory": c.TOL, "gradient, per block": c.TOL}


def _judge_row(worst, got, o, blks, at):
    """one trajectory: dict(loss, grad, x, u) of the kernel against the oracle's"""
    for k in ("loss", "grad", "x", "u"):
        assert np.isfinite(got[k]).all(), (at, k)
    worst.add("loss (relative)", abs(got["loss"] - o["loss"]) / abs(o["loss"]), at)
    worst.add("state trajectory", c.rel(got["x"], o["x"]), at)
    worst.add("control trajectory", c.rel(got["u"], o["u"]), at)
    worst.add("gradient, per block", c.block_rel(got["grad"], o["grad"], blks), at)


def _judge_case(res, worst, name, kind, key, T):
    blks = c.blocks(name, kind, key)
    p = c.n_params(name, kind, key)
    n, m = c.MODELS[name]
    for per_sample in (0, 1):
        k = _key(kind, name, key, T, per_sample)
        assert res[k + "loss"].shape == (c.B_UNIT,) and res[k + "grad"].shape == (c.B_UNIT, p) and res[k + "x"].shape == (c.B_UNIT, T + 1, n) and res[k + "u"].shape == (c.B_UNIT, T, m)
        assert res[k + "same"].all(), "%s: the call without trajectory outputs differs in (loss, gradient): %s" % (k, res[k + "same"])
        for b in range(c.B_UNIT):
            o = c.oracle_step(name, kind, key, T, bool(per_sample), b)
            _judge_row(worst, {q: res[k + q][b] for q in ("loss", "grad", "x", "u")}, o, blks,
                       "%s %s T=%d, %s theta, sample %d" % (kind, key, T, "per-sample" if per_sample else "shared", b))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("tag", POLY_TAGS)
def test_lagrange_policy_follows_the_oracle(run, margins, tag, name):
    res = run(tag)
    worst = _Worst()
    for _, N, T in c.poly_cases(name):
        _judge_case(res, worst, name, "poly", N, T)
        if tag == "given":
            assert int(res["ws|" + _key("poly", name, N, T)]) == c.prepass_ws_bytes(name, c.B_UNIT, T), (name, N, T)
    worst.check(margins, "%s %s Lagrange policy [%s]" % (tag, name, KERNELS[tag, "poly"]), BOUNDS)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("tag", MLP_TAGS)
def test_network_policy_follows_the_oracle(run, margins, tag, name):
    res = run(tag)
    worst = _Worst()
    for _, layers, T in c.mlp_cases(name, MLP_ROUTES[tag]):
        _judge_case(res, worst, name, "mlp", layers, T)
    worst.check(margins, "%s %s network policy [%s]" % (tag, name, KERNELS[tag, "mlp"]), BOUNDS)


@pytest.mark.parametrize("name", ("C16", "C5"))
def test_policies_handed_to_the_generic_kernel_follow_the_oracle(run, margins, name):
    """p > 512 (a shape the register kernels would take), width 33, nine layers: status 0 (the child's runtime.check) and the same bounds"""
    res = run("default")
    worst = _Worst()
    cases = c.mlp_cases(name, ("generic",))
    assert len(cases) == {"C16": 1, "C5": 2}[name] * len(c.MLP_HORIZONS)
    for _, layers, T in cases:
        _judge_case(res, worst, name, "mlp", layers, T)
    worst.check(margins, "default %s network policy handed over [cp_step_generic_kernel]" % name, BOUNDS)


def _big_rows(res, label, name):
    k = "big|%s|%s|" % (label, name)
    return int(res[k + "B"]), [int(r) for r in res[k + "rows"]], {q: res[k + q] for q in ("loss", "grad", "x", "u")}


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("tag", BIG_TAGS)
def test_lagrange_kernels_with_all_tiles_in_one_workgroup(run, margins, tag, name):
    """B = CUs + 1 and 2 CUs + 1 at T = 7, each model at its largest tile count: cp_step_poly2_kernel<NT, 2> and <NT, 4> with a ragged last workgroup under `pair`,
    cp_step_poly_kernel<NT> with every tile in one workgroup under `one_wave`, cp_poly_rollout_lanes_kernel over five and nine workgroups of 64 lanes (the last one
    with one trajectory) under `given`; rows 0, B // 2 and B - 1 against the oracle"""
    res = run(tag)
    cus = int(res["cus"])
    N, T = c.PAIR_PIVOTS[name], c.PAIR_T
    nt = c.tiles(N * c.MODELS[name][1])
    blks = c.blocks(name, "poly", N)
    theta = c.inputs(name, "poly", N, T)["theta"]
    worst = _Worst()
    for mult, tpw in ((1, 2), (2, 4)):
        B, rows, got = _big_rows(res, "B%d" % mult, name)
        assert B == mult * cus + 1 and c.traj_per_workgroup(B, cus) == tpw and B % tpw == 1 and rows == [0, B // 2, B - 1]
        assert c.split_tiles(nt, 2 * cus // B) == (1, nt)                                                      # the pair kernel: all tiles in one workgroup
        if mult == 2:
            assert c.split_tiles(nt, 4 * cus // B) == (1, nt)                                                  # and the one-wave kernel at 2 CUs + 1
        assert got["loss"].shape == (B,) and np.isfinite(got["loss"]).all() and np.isfinite(got["grad"]).all()
        x0 = c.big_rows(name, "poly", N, T, B)
        for i, b in enumerate(rows):
            o = c.oracle_step_at(name, "poly", N, T, x0[b], theta)
            _judge_row(worst, dict(loss=got["loss"][b], grad=got["grad"][b], x=got["x"][i], u=got["u"][i]), o, blks, "B = %d, row %d" % (B, b))
    worst.check(margins, "%s %s Lagrange policy, B = CUs + 1 and 2 CUs + 1, %d tiles per workgroup" % (tag, name, nt), BOUNDS)


def test_adjoint_kernel_with_offloaded_activations(run, margins):
    """C16 [12, 16, 4] at T = 65 under `one_wave`, at the smallest batch for which the restated cp_adjoint_plan offloads: rows 0, B // 2, B - 1 against the oracle, rows
    0 - 4 against the resident run at B = 5"""
    res = run("one_wave")
    cus = int(res["cus"])
    name, layers, T = c.OFFLOAD_CASE
    n = c.MODELS[name][0]
    p = c.mlp_params(n, layers)
    B, rows, got = _big_rows(res, "offload", name)
    info = c.generated_info(name)
    assert B == c.offload_batch(cus) and c.cp_adjoint_plan(info, layers, p, T, B, cus)[0] and not c.cp_adjoint_plan(info, layers, p, T, c.B_UNIT, cus)[0]
    assert int(res["offload_ws"]) >= B * T * sum(layers[:-1]) * 8
    blks = c.blocks(name, "mlp", layers)
    inp = c.inputs(name, "mlp", layers, T)
    x0 = c.big_rows(name, "mlp", layers, T, B)
    worst = _Worst()
    for i, b in enumerate(rows):
        if b >= c.B_UNIT:
            o = c.oracle_step_at(name, "mlp", layers, T, x0[b], inp["theta"])
        else:
            o = c.oracle_step(name, "mlp", layers, T, False, b)
        _judge_row(worst, dict(loss=got["loss"][b], grad=got["grad"][b], x=got["x"][i], u=got["u"][i]), o, blks, "B = %d, row %d" % (B, b))
    worst.check(margins, "one_wave C16 network [12, 16, 4] T=65 B=%d [cp_step_adjoint_kernel, activations offloaded]" % B, BOUNDS)
    k = _key("mlp", name, layers, T, 0)
    for b in range(c.B_UNIT):
        margins.check("cp edge offloaded vs resident adjoint kernel, row %d: gradient per block" % b, c.block_rel(got["grad"][b], res[k + "grad"][b], blks), c.TOL)
        margins.check("cp edge offloaded vs resident adjoint kernel, row %d: loss" % b, abs(got["loss"][b] - res[k + "loss"][b]) / abs(res[k + "loss"][b]), c.TOL_LOSS)


def _rel0(a, b):
    """max|a - b| / max|b|; an identically zero reference (d pi/dx of the open-loop Lagrange policy) asks for zeros"""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a).max()) if not np.abs(b).max() > 0 else c.rel(a, b)


@pytest.mark.parametrize("name", NAMES)
def test_class_surface_follows_the_oracle(run, margins, name):
    """integrateSys_batch, getAuxSys_batch and step_batch (cp_integrate_kernel, cp_auxsys_kernel, and the step kernel behind the class) for N = 6 and one network per model
    at T = 7, against the oracle's integrateSys, getAuxSys (dynF, dynG, dUx, dUe) and step: 1e-10 of each array's largest entry"""
    res = run("default")
    T = c.CLASS_T
    worst = _Worst()
    for kind, key in (("poly", 6), ("mlp", c.CLASS_MLP[name])):
        inp = c.inputs(name, kind, key, T)
        orc = c._oracle_with(name, kind, key, T)
        blks = c.blocks(name, kind, key)
        for per_sample in (0, 1):
            k = "class|" + _key(kind, name, key, T, per_sample)
            for b in range(c.B_UNIT):
                th = c.theta_of(inp, bool(per_sample), b)
                at = "%s %s, %s theta, sample %d" % (kind, key, "per-sample" if per_sample else "shared", b)
                sol = orc.integrateSys(inp["x0"][b], T, th)
                aux = orc.getAuxSys(sol["state_traj"], sol["control_traj"], th)
                o = c.oracle_step(name, kind, key, T, bool(per_sample), b)
                worst.add("integrateSys: state", c.rel(res[k + "x"][b], sol["state_traj"]), at)
                worst.add("integrateSys: control", c.rel(res[k + "u"][b], sol["control_traj"]), at)
                worst.add("integrateSys: cost", abs(res[k + "cost"][b] - sol["cost"]) / abs(sol["cost"]), at)
                for q in ("dynF", "dynG", "dUx", "dUe"):
                    worst.add("getAuxSys: " + q, _rel0(res[k + q][b], np.stack(aux[q])), at)
                worst.add("step: loss", abs(res[k + "loss"][b] - o["loss"]) / abs(o["loss"]), at)
                worst.add("step: gradient, per block", c.block_rel(res[k + "grad"][b], o["grad"], blks), at)
    worst.check(margins, "class surface %s [cp_integrate_kernel, cp_auxsys_kernel]" % name, dict.fromkeys(worst.v, c.TOL))


def test_register_kernels_equal_the_general_kernel(run):
    """csrc/pdp_cp_mlp_kernels.h / tests/test_gpu_cp_mlp.py on the new models: cp_step_mlp16_kernel (`pair`) against cp_step_adjoint_kernel (`one_wave`), and
    cp_step_mlp4t_kernel (`four`, shared theta) against cp_step_mlp16_kernel: loss and trajectories bit for bit, gradient to 1e-15 of its largest entry"""
    one, gen, four = run("pair"), run("one_wave"), run("four")
    differing = []
    for name, layers, T in c.mlp_cases(None, ("register",)):
        for per_sample in (0, 1):
            k = _key("mlp", name, layers, T, per_sample)
            for what, a, b in (("register kernel vs general kernel", one, gen), ("four-trajectory kernel vs register kernel", four, one)):
                for q in ("loss", "x", "u"):
                    if not np.array_equal(a[k + q], b[k + q]):
                        differing.append("%s %s%s: %.3e of the largest entry" % (what, k, q, c.rel(a[k + q], b[k + q])))
                e = max(c.rel(a[k + "grad"][i], b[k + "grad"][i]) for i in range(c.B_UNIT))
                if not e <= 1e-15:
                    differing.append("%s %sgrad: %.3e of the largest entry" % (what, k, e))
    assert not differing, "\n".join(differing)


def test_pair_kernel_equals_the_one_wave_kernel(run):
    """csrc/pdp_cp_pair_kernels.h / tests/test_gpu_cp_pair.py on the new models: loss, trajectories and gradient bit for bit - every Lagrange case at B = 5 (one tile per
    workgroup on both sides) and the large batches (all tiles in one workgroup; two and four trajectories per workgroup against one)"""
    pair, one = run("pair"), run("one_wave")
    keys = [_key("poly", name, N, T, ps) + q for name, N, T in c.poly_cases() for ps in (0, 1) for q in ("loss", "grad", "x", "u")]
    keys += ["big|B%d|%s|%s" % (mult, name, q) for mult in (1, 2) for name in NAMES for q in ("loss", "grad", "x", "u")]
    differing = []
    for k in keys:
        if not np.array_equal(pair[k], one[k]):
            d = np.abs(pair[k] - one[k])
            differing.append("%s: %d of %d entries, largest difference %.3e of the largest entry %.3e" % (k, int((d > 0).sum()), d.size, d.max(), np.abs(one[k]).max()))
    assert not differing, "\n".join(differing)


@pytest.mark.parametrize("tag", POLY_TAGS)
def test_argument_errors_write_nothing(run, tag):
    """17 pivots, and a parameter count that does not match the policy: PDP_E_ARG, with the 7.0-filled loss, gradient, trajectories and workspace untouched"""
    res = run(tag)
    for name in NAMES:
        for label in ("pivots17", "poly_p_plus_1", "poly_p_minus_1", "mlp_p_plus_1"):
            r = res["err|%s|%s" % (name, label)]
            assert r[0] == PDP_E_ARG and r[1:].all(), (tag, name, label, r)
