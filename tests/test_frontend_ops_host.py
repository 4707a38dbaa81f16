"""CPU: the symbolic front-end (pdp_amd.sx) and the code generator (pdp_amd.codegen) on models that use every operator the front-end offers - the models of
tests/frontend_ops_common.py - with sympy's derivatives evaluated in 40-digit arithmetic as the reference.  No GPU, no hipcc.

1. sx against sympy: values, sx.jacobian and sx.hessian through sx.Function, per entry relative to that entry's own magnitude, structural zeros exactly zero, <= REF_CAP.
2. The emitted C text as numbers: codegen.generate(problem)[0] compiled for the host (g++ -DPDP_HD=inline, a plain build) and called through ctypes - precompute
   [precompute_u], every function and every eval_<group> of the kind, the group's dense matrices assembled as the kernels' sinks do (put<k> scattered by <G>_MAT /
   <G>_OFF, the other entries from <g>_code / <g>_const).  This reads back the a / b(theta) -> a * (1 / b) rewrite, the hoisting into pc[], the code tables and the
   constant pools.  Same bound.
3. The conditions tests/test_gpu_frontend_ops.py rests on: every rollout it uses keeps every operator inside its domain; oracle.pdp_oc_unit agrees with the 40-digit
   solve to REF_CAP on every sample; no column of dx/dtheta is identically zero; the OPT points - x0, and x1 and op(x0) for the final cost - give fp64 values within REF_CAP of the 40-digit ones; the solver case converges in
   oracle.ipopt_ms.solve within MAX_ITER_ORACLE iterations, without a restoration, with no inertia correction in any iteration
   and H_uu positive definite at every stage of the optimum.
4. Generator facts of OPS5: hoisted values exist, the source calls pow, tan, exp, log and sqrt, a rewritten division is a product by a pc[] value."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import frontend_ops_common as c  # noqa: E402

KINDS = {"oc": 0, "cp": 1, "sysid": 2}
GROUPS = {"oc": dict(path=["F", "G", "E", "Hxx", "Hxu", "Hxe", "Huu", "Hue"], patha=["F", "G", "E", "cx"], pathb=["Hxx", "Hxu", "Hxe", "Huu", "Hue"], fwd=["F", "G", "E"],
                     fin=["hxx", "hxe"], sol=["F", "G", "Hxx", "Hxu", "Huu"], solf=["F", "G"]),
          "cp": dict(path=["F", "G", "cx", "cu"]), "sysid": dict(path=["F", "E"], pathu=["G"])}


def points(name, kind):
    """list of (x, u, lam, w): OPT at its table points (shared and per-sample parameters), the others at five draws of the unit-input recipe"""
    n, m, p = c.MODELS[name]
    if name == "OPT":
        P = c.opt_points()
        return [(P["x0"][b], P["u"][b, 0], P["lam"][b, 0], th) for b in range(P["B"]) for th in (P["theta"], P["theta_b"][b])]
    rng = np.random.default_rng(n)
    keep = {"oc": p, "sysid": c.SYSID_P, "cp": 0}[kind]
    return [(0.5 * rng.standard_normal(n), 0.3 * rng.standard_normal(m), rng.standard_normal(n), (c.NOMINAL[name] * (1 + 0.05 * rng.standard_normal(p)))[:keep]) for _ in range(5)]


# ---- 1. sx against sympy ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", c.LIBRARIES)
def test_sx_values_jacobians_and_hessians_follow_sympy(name, kind):
    from pdp_amd import sx
    xs, us, ws, f, path, final = c.kind_equations(name, kind, "sx")
    mats, lams = c._matrices("sx", kind, xs, us, ws, f, path, final)
    keys = sorted(mats)
    fn = sx.Function("f", [sx.vertcat(*xs), sx.vertcat(*us), sx.vertcat(*lams), sx.vertcat(*ws) if ws else sx.SX()], [mats[k] for k in keys])
    worst = c.Worst()
    for i, (x, u, lam, w) in enumerate(points(name, kind)):
        ex = c.exact(name, kind, x, u, lam, w)
        got = fn(x, u, lam, w)
        got = got if isinstance(got, tuple) else (got,)
        for k, g in zip(keys, got):
            worst.add(k, c.entry_err(g.full(), *ex[k]), i)
    for k, (e, i) in sorted(worst.v.items()):
        print("%s %s: sx.Function %s vs sympy at %d digits, worst entry %.2e (point %d)" % (name, kind, k, c.DPS, e, i))
    for k, (e, i) in worst.v.items():
        assert e <= c.REF_CAP, (name, kind, k, e, i)


# ---- 2. the emitted C text ----------------------------------------------------------------------------------------------------------------------------------
HARNESS = r"""
#include <cmath>
using std::pow;
#define PDP_HD inline
namespace {              // internal linkage: a second model's library in the same process must not bind to this one's tables
#include "model.h"
}
struct Sink { double* v; template <int K> void put(double e) { v[K] = e; } };
#define GROUP(g, G) \
    int g##_nvar() { return PdpModel::G##_NVAR; } \
    int g##_nmat() { return PdpModel::G##_NMAT; } \
    int g##_nconst() { return PdpModel::G##_NCONST; } \
    int g##_rows(int i) { return PdpModel::G##_ROWS[i]; } \
    int g##_cols(int i) { return PdpModel::G##_COLS[i]; } \
    int g##_mat(int k) { return PdpModel::G##_MAT[k]; } \
    int g##_off(int k) { return PdpModel::G##_OFF[k]; } \
    int g##_code(int mat, int i) { return PdpModel::g##_code(mat, i); } \
    double g##_const(int k) { return PdpModel::g##_const(k); } \
    void g##_eval(const double* x, const double* u, const double* lam, const double* th, const double* pc, double* v) { Sink s{v}; PdpModel::eval_##g(x, u, lam, th, pc, s); }
extern "C" {
int sizes(int i) { const int s[] = {PdpModel::KIND, PdpModel::NX, PdpModel::NU, PdpModel::NP, PdpModel::NPC}; return s[i]; }
void precompute(const double* th, double* pc) { PdpModel::precompute(th, pc); }
void dyn(const double* x, const double* u, const double* th, const double* pc, double* out) { PdpModel::dyn(x, u, th, pc, out); }
GROUP(path, PATH)
#if HKIND != 2
double path_cost(const double* x, const double* u, const double* th, const double* pc) { return PdpModel::path_cost(x, u, th, pc); }
double final_cost(const double* x, const double* th, const double* pc) { return PdpModel::final_cost(x, th, pc); }
void dhx(const double* x, const double* th, const double* pc, double* out) { PdpModel::dhx(x, th, pc, out); }
#endif
#if HKIND == 0
void costate_step(const double* x, const double* u, const double* lam, const double* th, const double* pc, double* out) { PdpModel::costate_step(x, u, lam, th, pc, out); }
void dHu(const double* x, const double* u, const double* lam, const double* th, const double* pc, double* out) { PdpModel::dHu(x, u, lam, th, pc, out); }
GROUP(patha, PATHA) GROUP(pathb, PATHB) GROUP(fwd, FWD) GROUP(fin, FIN) GROUP(sol, SOL) GROUP(solf, SOLF)
#endif
#if HKIND == 2
int npcu() { return PdpModel::NPCU; }
void precompute_u(const double* th, double* pc) { PdpModel::precompute_u(th, pc); }
GROUP(pathu, PATHU)
#endif
}
"""


def _host_library(name, kind, tmp):
    src = c.generated(name, kind)[0]
    with open(os.path.join(tmp, "model.h"), "w") as f:
        f.write(src)
    with open(os.path.join(tmp, "harness.cpp"), "w") as f:
        f.write(HARNESS)
    so = os.path.join(tmp, "libmodel_host.so")
    # -ffp-contract=off: the reference is the text's value, operation by operation
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-DHKIND=%d" % KINDS[kind], "-I", tmp, "-o", so, os.path.join(tmp, "harness.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return ctypes.CDLL(so)


def _arr(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    if a.size == 0:
        a = np.zeros(1)
    return a


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _group_matrices(lib, g, x, u, lam, th, pc):
    """the dense matrices of one group, assembled as a kernel's sink does: NaN everywhere, put<k> scattered to (<G>_MAT[k], <G>_OFF[k]); then every entry read through
    <g>_code: -1 a zero, -2 - c the constant c, k the value of put<k>"""
    I = lambda fn, *a: int(getattr(lib, "%s_%s" % (g, fn))(*a))
    getattr(lib, g + "_const").restype = ctypes.c_double
    nvar, nmat = I("nvar"), I("nmat")
    v = np.full(max(1, nvar), np.nan)
    getattr(lib, g + "_eval")(_p(x), _p(u), _p(lam), _p(th), _p(pc), _p(v))
    assert np.isfinite(v[:nvar]).all(), (g, v)              # every put<k> was called
    shapes = [(I("rows", i), I("cols", i)) for i in range(nmat)]
    scattered = [np.full(r * cc, np.nan) for r, cc in shapes]
    for k in range(nvar):
        mi, off = I("mat", k), I("off", k)
        assert 0 <= mi < nmat and 0 <= off < scattered[mi].size and np.isnan(scattered[mi][off]), (g, k, mi, off)      # one element per slot, none twice
        scattered[mi][off] = v[k]
        assert I("code", mi, off) == k
    dense, zeros = [], []
    for mi, (r, cc) in enumerate(shapes):
        M, Z = np.zeros(r * cc), np.zeros(r * cc, dtype=bool)
        for i in range(r * cc):
            code = I("code", mi, i)
            assert -2 - I("nconst") < code < nvar, (g, mi, i, code)
            if code == -1:
                Z[i] = True
            elif code <= -2:
                M[i] = getattr(lib, g + "_const")(-2 - code)
                assert M[i] != 0.0
            else:
                M[i] = v[code]
                assert np.isnan(scattered[mi][i]) or scattered[mi][i] == v[code]
        dense.append(M.reshape(r, cc))
        zeros.append(Z.reshape(r, cc))
    return dense, zeros


@pytest.mark.parametrize("name,kind", c.LIBRARIES)
def test_emitted_c_text_evaluates_to_sympys_numbers(name, kind, tmp_path):
    lib = _host_library(name, kind, str(tmp_path))
    n, m, p = c.MODELS[name]
    p = {"oc": p, "sysid": c.SYSID_P, "cp": 0}[kind]
    assert [lib.sizes(i) for i in range(4)] == [KINDS[kind], n, m, p]
    npc = lib.sizes(4)
    assert npc == max(1, c.generated_info(name, kind)["npc"])
    for fn in ("path_cost", "final_cost"):
        if kind != "sysid":
            getattr(lib, fn).restype = ctypes.c_double
    worst = c.Worst()
    for i, (x, u, lam, w) in enumerate(points(name, kind)):
        ex = c.exact(name, kind, x, u, lam, w)
        x, u, lam, th = _arr(x), _arr(u), _arr(lam), _arr(w)
        pc = np.full(npc + 1, np.nan)
        lib.precompute(_p(th), _p(pc))
        assert np.isnan(pc[npc]) and (np.isfinite(pc[:npc]).all() or c.generated_info(name, kind)["npc"] == 0)
        got = {}
        out = np.full(n + 1, np.nan)
        lib.dyn(_p(x), _p(u), _p(th), _p(pc), _p(out))
        got["dyn"] = out[:n].copy()
        assert np.isnan(out[n])
        if kind != "sysid":
            got["path_cost"], got["final_cost"] = lib.path_cost(_p(x), _p(u), _p(th), _p(pc)), lib.final_cost(_p(x), _p(th), _p(pc))
            lib.dhx(_p(x), _p(th), _p(pc), _p(out))
            got["dhx"] = out[:n].copy()
        if kind == "oc":
            lib.costate_step(_p(x), _p(u), _p(lam), _p(th), _p(pc), _p(out))
            got["costate_step"] = out[:n].copy()
            outu = np.full(m, np.nan)
            lib.dHu(_p(x), _p(u), _p(lam), _p(th), _p(pc), _p(outu))
            got["dHu"] = outu
        for k, g in got.items():
            worst.add(k, c.entry_err(g, *ex[k]), i)
        for g, names in GROUPS[kind].items():
            pcg = pc
            if g == "pathu":
                pcg = np.full(lib.npcu() + 1, np.nan)
                lib.precompute_u(_p(th), _p(pcg))
                assert np.isnan(pcg[-1]) and np.array_equal(pcg[:npc], pc[:npc])               # the values of precompute first, unchanged
            dense, zeros = _group_matrices(lib, g, x, u, lam, th, pcg)
            assert len(dense) == len(names)
            for k, M, Z in zip(names, dense, zeros):
                want, zero = ex[k]
                assert M.shape == want.shape, (g, k, M.shape, want.shape)
                assert np.array_equal(Z, zero), (name, kind, g, k, "the code table's zeros are not sympy's structural zeros")
                worst.add("%s.%s" % (g, k), c.entry_err(M, want, zero), i)
    for k, (e, i) in sorted(worst.v.items()):
        print("%s %s: emitted C %s vs sympy at %d digits, worst entry %.2e (point %d)" % (name, kind, k, c.DPS, e, i))
    for k, (e, i) in worst.v.items():
        assert e <= c.REF_CAP, (name, kind, k, e, i)


# ---- 3. the conditions the GPU tests rest on ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("OPS5", "OPS3"))
def test_unit_rollouts_stay_inside_every_domain_and_the_reference_order_is_accurate(name):
    for T in c.unit_horizons(name):
        inp = c.unit_inputs(name, T)
        for per_sample in (False, True):
            worst_d = None
            for b in range(c.B):
                o = c.unit_oracle(name, T, per_sample, b)
                d = c.in_domain(name, o["state_traj"], inp["u"][b], c.theta_of(inp, per_sample, b))
                assert c.domain_ok(d), (name, T, per_sample, b, d)
                assert np.isfinite(o["state_traj"]).all() and np.isfinite(o["costate_traj"]).all() and np.isfinite(o["grad"]).all()
                worst_d = d if worst_d is None else dict(base=min(d["base"], worst_d["base"]), **{k: max(d[k], worst_d[k]) for k in ("tan", "exp", "tanh")})
            print("%s T=%d %s theta: smallest log / sqrt / pow base %.3f, largest |tan arg| %.3f, |exp arg| %.3f, |x| %.3f" %
                  (name, T, "per-sample" if per_sample else "shared", worst_d["base"], worst_d["tan"], worst_d["exp"], worst_d["tanh"]))
            for b in range(c.B):
                o = c.unit_oracle(name, T, per_sample, b)
                Xe, Ue = c.unit_exact(name, T, per_sample, b)
                ex, eu = c.rel(np.stack(o["lqr"]["state_traj_opt"]), Xe), c.rel(np.stack(o["lqr"]["control_traj_opt"]), Ue)
                huu = min(np.linalg.eigvalsh(np.asarray(h, float)).min() for h in o["aux"]["Huu"])
                print("%s T=%d %s theta sample %d: reference order vs %d digits X %.2e U %.2e (smallest eigenvalue of H_uu %.3f)" %
                      (name, T, "per-sample" if per_sample else "shared", b, c.DPS, ex, eu, huu))
                assert ex <= c.REF_CAP and eu <= c.REF_CAP, (name, T, per_sample, b, ex, eu)


@pytest.mark.parametrize("name", ("OPS5", "OPS3"))
def test_every_parameter_moves_the_trajectory(name):
    Xe, Ue = c.unit_exact(name, 7, False, 0)
    assert (np.abs(Xe).max(axis=(0, 1)) > 0).all() and (np.abs(Ue).max(axis=(0, 1)) > 0).all()


def test_sysid_and_control_planning_rollouts_stay_inside_every_domain():
    assert c.generated_info("OPS5", "cp")["nvar"]["path"] == c.CP_PATH_NVAR and c.cp_horizons() == (7, c.CP_ROWS + 1)
    for T in c.sysid_horizons():
        cs = c.sysid_case(T)
        for per_sample in (False, True):
            for b in range(c.B):
                r = c.sysid_reference(T, per_sample, b)
                w = np.concatenate([cs["theta_b"][b] if per_sample else cs["theta"], c.NOMINAL["OPS5"][c.SYSID_P:]])
                d = c.in_domain("OPS5", r["x"], cs["inputs"][b], w)
                assert c.domain_ok(d) and all(np.isfinite(r[k]).all() for k in ("grad", "gn", "grad_u", "d_x")), ("sysid", T, per_sample, b, d)
                assert (np.abs(r["X"]).max(axis=(0, 1)) > 0).all()                 # every parameter moves the rollout
        print("OPS5 SysID T=%d: max|x| %.3f" % (T, max(np.abs(c.sysid_reference(T, ps, b)["x"]).max() for ps in (False, True) for b in range(c.B))))
    for policy in ("poly", "mlp"):
        for T in c.cp_horizons():
            for per_sample in (False, True):
                for b in range(c.B):
                    r = c.cp_reference(policy, T, per_sample, b)
                    d = c.in_domain("OPS5", r["x"], r["u"], c.NOMINAL["OPS5"])
                    assert c.domain_ok(d) and np.isfinite(r["step_grad"]).all() and np.abs(r["step_grad"]).min() > 0, ("cp", policy, T, per_sample, b, d)
            print("OPS5 CP %s T=%d: max|x| %.3f, max|u| %.3f" % (policy, T, max(np.abs(c.cp_reference(policy, T, ps, b)["x"]).max() for ps in (False, True) for b in range(c.B)),
                                                                   max(np.abs(c.cp_reference(policy, T, ps, b)["u"]).max() for ps in (False, True) for b in range(c.B))))


def test_operator_table_points_are_well_conditioned():
    """every non-structural entry at every point tests/test_gpu_frontend_ops.py evaluates OPT at - (x0, u, lam) for every quantity, x1 and op(x0) for what belongs to the
    final cost, shared and per-sample parameters: pdp_amd.sx's host fp64 value (the un-rewritten expression) is finite and within REF_CAP of the 40-digit one, so no entry
    is the small difference of large terms - and the rows the table is there for are present: negative bases under the odd powers"""
    from pdp_amd import sx
    P = c.opt_points()
    for i in (1, 8, 9, 10):
        assert (P["x0"][:, i] < 0).sum() >= 3 and (P["x0"][:, i] > 0).any()
    assert (P["x0"][:, [5, 6, 7, 12]] >= 1e-3).all() and (np.abs(P["x0"][:, 3]) <= 1.4).all() and (np.abs(P["x0"][:, 5]) <= 20).all() and (np.abs(P["x0"][:, 4]) <= 3).all()
    xs, us, ws, f, path, final = c.equations("OPT", "sx")
    mats, lams = c._matrices("sx", "oc", xs, us, ws, f, path, final)
    args = [sx.vertcat(*xs), sx.vertcat(*us), sx.vertcat(*lams), sx.vertcat(*ws)]
    keys = sorted(mats)
    fn, fin = sx.Function("all", args, [mats[k] for k in keys]), sx.Function("fin", args, [mats[k] for k in c.FINAL_KEYS])
    worst, big, small = c.Worst(), 0.0, np.inf
    for b in range(P["B"]):
        for mode, w in (("shared", P["theta"]), ("per-sample", P["theta_b"][b])):
            at = "%s theta, row %d" % (mode, b)
            u, lam = P["u"][b, 0], P["lam"][b, 0]
            e0 = c.exact("OPT", "oc", P["x0"][b], u, lam, w)
            for k, g in zip(keys, fn(P["x0"][b], u, lam, w)):
                worst.add("at x0: " + k, c.entry_err(g.full(), *e0[k]), at)
                a = np.abs(e0[k][0][~e0[k][1]])
                if a.size:
                    assert (a > 0).all(), (k, at)
                    big, small = max(big, a.max()), min(small, a.min())
            for label, x in (("at x1: ", P["x1"][b]), ("at op(x0): ", e0["dyn"][0][:, 0])):
                e1 = c.exact("OPT", "oc", x, u, lam, w, final_only=True)
                for k, g in zip(c.FINAL_KEYS, fin(x, u, lam, w)):
                    worst.add(label + k, c.entry_err(g.full(), *e1[k]), at)
    print("OPT: non-structural entries at x0 between %.3e and %.3e" % (small, big))
    for k, (e, at) in sorted(worst.v.items()):
        print("OPT %s: host fp64 vs %d digits, worst entry %.2e (%s)" % (k, c.DPS, e, at))
    for k, (e, at) in worst.v.items():
        assert e <= c.REF_CAP, (k, e, at)


def test_solver_case_converges_with_positive_definite_huu():
    oc = c.model_oracle("OPS5")
    th = c.solver_theta()
    for row in range(len(c.solver_x0())):
        ref, log = c.solver_oracle(row)
        xs, us, lam = ref["state_traj_opt"], ref["control_traj_opt"], ref["costate_traj_opt"]
        aux = oc.getAuxSys(xs, us, lam, th)
        huu = min(np.linalg.eigvalsh(h).min() for h in aux["Huu"])
        d = c.in_domain("OPS5", xs, us, th)
        print("OPS5 solver row %d: %d iterations, %d restorations, dw > 0 on %d, alpha < 1 on %d, smallest eigenvalue of H_uu at the optimum %.3f, max|x| %.2f" %
              (row, ref["iterations"], ref["restorations"], sum(l["dw"] > 0 for l in log), sum(l["alpha"] < 1 for l in log), huu, d["tanh"]))
        assert ref["iterations"] == len(log) <= c.MAX_ITER_ORACLE and ref["restorations"] == 0
        assert all(l["dw"] == 0.0 for l in log), "an inertia correction: H_uu was not positive definite along the iterates"
        assert huu > 0 and c.domain_ok(d)


# ---- 4. generator facts -------------------------------------------------------------------------------------------------------------------------------------
def test_generator_facts_of_ops5():
    src, info = c.generated("OPS5", "oc")
    assert info["npc"] > 0 and (info["n"], info["m"], info["p"]) == c.MODELS["OPS5"]
    for call in ("pow(", "tan(", "exp(", "log(", "sqrt("):
        assert call in src, call
    # u1 / exp(w3): the divisor is theta-only, so no statement divides by it outside precompute and some statement multiplies by a pc[] value
    body = src.split("static void dyn(")[1].split("}")[0]
    assert re.search(r"\* pc\[\d+\]|pc\[\d+\] \*", body), body
    assert not re.search(r"/ (th|pc)\[", src.split("static void dyn(")[1]), "a division by a theta-only value outside precompute"
    pre = src.split("static void precompute(")[1].split("}")[0]
    assert "exp(" in pre and "sqrt(" in pre and "1.0 / " in pre
    sid_src, sid = c.generated("OPS5", "sysid")
    npcu = int(re.search(r"NPCU = (\d+)", sid_src).group(1))
    print("OPS5: OC NPC %d, %d path entries; SysID NPC %d, NPCU %d" % (info["npc"], info["nvar"]["path"], sid["npc"], npcu))
    assert npcu >= sid["npc"] > 0
