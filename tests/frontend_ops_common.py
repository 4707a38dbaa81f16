"""Shared by tests/test_frontend_ops_host.py (CPU) and tests/test_gpu_frontend_ops.py (GPU): user models that use every operator the symbolic front-end
(pdp_amd.sx) offers, so that the code pdp_amd.codegen emits for them - derivative rules, the device pow, the a / b(theta) -> a * (1 / b) rewrite, the theta-only values
hoisted into precompute - is evaluated as numbers.  The zoo and the other test models reach sin, cos, tanh, log and division by a mass matrix only.

    name   n  m   p   what it is
    OPS5   5  2   8   the issue's five-state model (equations below): tan, exp, log, sqrt, tanh, sin, cos, pow with the exponents 1.5, 2.5, -0.5, -2, 5 and two variable
                      exponents (one a parameter, one a function of the state), divisions by functions of the state, of the control and of the parameters, and
                      theta-only transcendental values (exp(w3), sqrt(w1^2 + 1), 1 / (8 w2), 1 / (4 w7)).  The same equations as OC, as SysID (the dynamics with
                      auxvar w0..w4, the rest as numbers) and as ControlPlanning (all parameters as numbers).
    OPS3   3  2   5   a three-state reduction from the same operator families, for the small-system kernels (n <= 4: the one-wave kernel, pdp_riccati_small.h).
    OPT   16  4  12   the operator table: x_i+ = op_i(x_i [, w, u]) with NO x_i + dt (...) in front, the costs sums of single operators of single variables, evaluated
                      at T = 1 with the batch rows as argument points - an entry of F, G, E, H.., h.. is one operator's first or second derivative (or lam_i times one
                      plus a cost term's).  Rows: every name of sx._UNARY and sx._BINARY; every exponent sx.powr special-cases (0, 1, 2, 3, 4, -1, -2, 0.5) and 1.5,
                      -0.5 beside them; 5, 7 and -3 at negative bases; x^w and w^x; x / w (rewritten), x / u, x / (1 + x'^2), w / x; sin(-x), tan(-x), tanh(-x),
                      cos(-x); a theta-only row exp(w3) sqrt(1 + w4^2); norm_2; a 2 x 2 sx.inv with state-dependent entries.

The equations are written once against lists of scalars and a namespace `S` of functions (sympy_namespace / sx_namespace), so pdp_amd.sx and sympy are given the same
expressions.  The reference of every single evaluation is sympy's derivative evaluated in 40-digit arithmetic (exact()); trajectories are compared with
oracle.pdp_oracle (fp64, the reference's order), whose own error against 40 digits tests/test_frontend_ops_host.py bounds by REF_CAP."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import tile_edge_common as te  # noqa: E402

TOL, REF_CAP = te.TOL, te.REF_CAP
MAX_ITER_ORACLE = te.MAX_ITER_ORACLE
DPS = 40
B = 5
MODELS = {"OPS5": (5, 2, 8), "OPS3": (3, 2, 5), "OPT": (16, 4, 12)}
DT = 0.1
NOMINAL = {"OPS5": np.array([0.5, 0.8, 1.2, 0.7, 0.6, 1.0, 0.5, 0.4]), "OPS3": np.array([0.5, 0.8, 1.2, 0.7, 0.4]),
           "OPT": np.array([0.7, 1.6, 1.3, 0.4, 0.9, 1.1, 0.8, 1.2, 0.6, 1.4, 0.5, 0.9])}
SYSID_P = 5                  # OPS5 as SysID: auxvar w0..w4 (the parameters of the dynamics), w5..w7 are the cost's
W7_SOLVER = 4.0              # OPS5, the solver case: H_uu is positive definite along the oracle's iterates (tests/test_frontend_ops_host.py measures it)
SOLVER_T = 12


# ---- the two libraries --------------------------------------------------------------------------------------------------------------------------------------
def sympy_namespace():
    import sympy as sp

    class S:
        sin, cos, tan, tanh, exp, log, sqrt = sp.sin, sp.cos, sp.tan, sp.tanh, sp.exp, sp.log, sp.sqrt

        @staticmethod
        def norm_2(v):
            return sp.sqrt(sum(e * e for e in v))

        @staticmethod
        def inv2(a, b, c, d):
            """the four entries (row-major) of the inverse of [[a, b], [c, d]]"""
            M = sp.Matrix([[a, b], [c, d]]).inv()
            return [M[0, 0], M[0, 1], M[1, 0], M[1, 1]]
    return S


def sx_namespace():
    from pdp_amd import sx

    class S:
        sin, cos, tan, tanh, exp, log, sqrt = sx.sin, sx.cos, sx.tan, sx.tanh, sx.exp, sx.log, sx.sqrt

        @staticmethod
        def norm_2(v):
            return sx.norm_2(sx.vertcat(*v))

        @staticmethod
        def inv2(a, b, c, d):
            M = sx.inv(sx.vertcat(sx.horzcat(a, b), sx.horzcat(c, d)))
            return [M[0, 0], M[0, 1], M[1, 0], M[1, 1]]
    return S


def _symbols(name, lib):
    n, m, p = MODELS[name]
    if lib == "sx":
        from pdp_amd.sx import SX
        X, U, w = SX.sym("x", n), SX.sym("u", m), SX.sym("w", p)
        return sx_namespace(), [X[i] for i in range(n)], [U[i] for i in range(m)], [w[i] for i in range(p)]
    import sympy as sp
    return (sympy_namespace(),) + tuple(list(sp.symbols("%s0:%d" % (s, k), real=True)) for s, k in (("x", n), ("u", m), ("w", p)))


def _ops5(S, x, u, w):
    dt = DT
    r = S.sqrt(1.0 + x[0] * x[0] + x[1] * x[1])
    f = [x[0] + dt * (-x[0] + S.tan(0.4 * S.tanh(x[1])) + S.exp(-w[0] * x[2] * x[2]) * u[0] / r),
         x[1] + dt * (-x[1] + S.log(2.0 + w[1] * w[1] + x[0] * x[0]) - (2.0 + x[2] * x[2]) ** 1.5 / (8.0 * w[2]) + u[1] / S.exp(w[3])),
         x[2] + dt * (-x[2] + (1.5 + S.tanh(x[0])) ** w[3] - x[1] / (3.0 + S.cos(u[0])) + (S.sqrt(w[1] * w[1] + 1.0) - 1.0) * x[3]),
         x[3] + dt * (-w[4] * x[3] + (1.0 + x[4] * x[4]) ** (-0.5) + S.sin(-x[2]) * (w[0] + 1.0) ** (0.3 * S.tanh(x[1]))),
         x[4] + dt * (-x[4] + S.tanh(-x[3]) * S.cos(-x[0]) + u[0] * u[1] / (w[2] + x[1] * x[1]) + (2.0 + S.sin(x[2])) ** 5 / 100.0)]
    path = (w[5] * x[0] * x[0] + w[6] * S.exp(0.3 * x[1]) + (1.0 + x[2] * x[2]) ** 2.5 + w[7] * (u[0] * u[0] + u[1] * u[1]) + 1.0 / (1.0 + x[3] * x[3])
            + (2.0 + x[4] * x[4]) ** (-2) - S.log(1.0 + u[0] * u[0]) / (4.0 * w[7]) + 0.1 * w[5] * S.sqrt(1.0 + x[3] * x[3] + x[4] * x[4]) + S.tan(0.2 * x[4]) ** 2)
    final = w[5] * S.exp(0.1 * x[0]) + w[6] * (1.0 + x[1] * x[1]) ** 1.5 + S.log(1.0 + x[2] * x[2] + x[3] * x[3]) + x[4] ** 4
    return f, path, final


def _ops3(S, x, u, w):
    dt = DT
    r = S.sqrt(1.0 + x[0] * x[0] + x[1] * x[1])
    f = [x[0] + dt * (-x[0] + S.tan(0.4 * S.tanh(x[1])) + S.exp(-w[0] * x[2] * x[2]) * u[0] / r),
         x[1] + dt * (-x[1] + S.log(2.0 + w[1] * w[1] + x[0] * x[0]) - (2.0 + x[2] * x[2]) ** 1.5 / (8.0 * w[2]) + u[1] / S.exp(w[3])),
         x[2] + dt * (-x[2] + (1.5 + S.tanh(x[0])) ** w[3] - x[1] / (3.0 + S.cos(u[0])) + S.sin(-x[2]) * (w[0] + 1.0) ** (0.3 * S.tanh(x[1]))
                      + (S.sqrt(w[1] * w[1] + 1.0) - 1.0) * S.cos(-x[0]) + (2.0 + S.sin(x[1])) ** 5 / 100.0)]
    path = (w[1] * x[0] * x[0] + w[2] * S.exp(0.3 * x[1]) + (1.0 + x[2] * x[2]) ** 2.5 + w[4] * (u[0] * u[0] + u[1] * u[1]) + 1.0 / (1.0 + x[0] * x[0])
            + (2.0 + x[1] * x[1]) ** (-2) - S.log(1.0 + u[0] * u[0]) / (4.0 * w[4]) + 0.1 * w[1] * (1.0 + x[1] * x[1] + x[2] * x[2]) ** (-0.5) + S.tan(0.2 * x[2]) ** 2)
    final = w[1] * S.exp(0.1 * x[0]) + w[2] * (1.0 + x[1] * x[1]) ** 1.5 + S.log(1.0 + x[2] * x[2]) + x[0] ** 4
    return f, path, final


def _opt(S, x, u, w):
    """the operator table.  State domains (opt_points): x5 in (0, 3) (exp, x^0.5), x6, x7, x12 > 0 (log and x^1.5, sqrt, x^w and x^-0.5), |x3| <= 1.3 and not 0 (tan, 1 / x), x4, x15 not 0 (x^-2, w / x),
    x1, x8, x9, x10 negative in some rows (the odd powers), u3 not 0 (x / u)"""
    f = [-x[0],                                            # neg
         S.sin(x[1]), S.cos(x[2]), S.tan(x[3]), S.tanh(x[4]), S.exp(x[5]), S.log(x[6]), S.sqrt(x[7]),
         x[8] + u[0],                                      # add
         x[9] - u[1],                                      # sub
         x[10] * u[2],                                     # mul
         x[11] / u[3],                                     # div by a control: stays a division
         x[12] ** w[0],                                    # pow, the exponent a parameter
         w[1] ** x[13],                                    # pow, the base a parameter
         x[14] / w[2],                                     # div by a parameter: rewritten to x * (1 / w), the reciprocal hoisted
         S.exp(w[3]) * S.sqrt(1.0 + w[4] * w[4])]          # theta-only: the output is itself a hoisted value
    iv = S.inv2(2.0 + x[2] * x[2], x[3], S.sin(x[4]), 3.0 + x[5] * x[5])
    path = (w[5] * x[0] ** 0 + x[11] ** 1 + x[0] ** 2 + x[1] ** 3 + x[2] ** 4 + x[3] ** (-1) + x[4] ** (-2) + x[5] ** 0.5                     # the special-cased exponents
            + x[6] ** 1.5 + x[12] ** (-0.5) + x[8] ** 5 + x[9] ** 7 + x[10] ** (-3)                                                             # pow(): the last three at negative bases
            + w[6] * S.sin(-u[0]) + w[7] * S.tan(-u[1]) + S.tanh(-u[2]) / w[8] + S.cos(-u[3]) * S.exp(0.5 * u[0])                                # the sign-pulling rules, on the controls
            + x[13] / (1.0 + x[14] * x[14]) + w[9] / x[15]
            + S.norm_2([x[0], x[8], u[1]])
            + w[10] * (iv[0] + 2.0 * iv[1] + 3.0 * iv[2] + 4.0 * iv[3])
            + S.log(2.0 + u[2] * u[2]) * w[11] + S.sqrt(1.0 + u[3] * u[3]) + (1.0 + u[1] * u[1]) ** 1.5)
    # evaluated at op(x): every term is defined on the whole real line
    final = (w[5] * S.exp(0.1 * x[0]) + S.sin(x[1]) * w[6] + x[2] ** 3 + S.tanh(x[3]) + x[4] ** 5 + S.log(1.0 + x[5] * x[5]) + (1.0 + x[6] * x[6]) ** 1.5 + S.cos(x[7]) / w[7]
             + x[8] ** 4 + (2.0 + x[9] * x[9]) ** (-0.5) + S.sqrt(1.0 + x[10] * x[10]) + x[11] ** 2 + S.log(1.0 + x[12] * x[12]) * w[8] + S.tanh(0.01 * x[13]) + x[14] ** 7 * 1e-3
             + x[15] * x[15] * w[9])
    return f, path, final


_EQ = {"OPS5": _ops5, "OPS3": _ops3, "OPT": _opt}


def equations(name, lib, theta=None, keep=None):
    """(state, control, auxvar, dynamics, path cost, final cost) as lists of scalars / scalars of the symbolic library `lib` ("sx": pdp_amd.sx, else sympy).
    theta [p] with keep = k: the parameters from w_k on are replaced by these doubles (tile_edge_common.equations: pdp_amd.sx.substitute / sympy's .subs of the double
    carried at 40 digits) and the auxvar that comes back is w_0 .. w_{k-1} (ControlPlanning: keep = 0; SysID: keep = SYSID_P)"""
    S, xs, us, ws = _symbols(name, lib)
    f, path, final = _EQ[name](S, xs, us, ws)
    if theta is None:
        return xs, us, ws, f, path, final
    keep = 0 if keep is None else keep
    vals = [float(v) for v in theta][keep:]
    assert len(theta) == len(ws)
    if not vals:
        return xs, us, ws, f, path, final
    if lib == "sx":
        from pdp_amd import sx
        old, new = sx.vertcat(*ws[keep:]), sx.SX(np.array(vals).reshape(-1, 1))
        sub = lambda e: sx.substitute(e, old, new)
        return xs, us, ws[:keep], [sub(fi) for fi in f], sub(path), sub(final)
    import sympy as sp
    rep = dict(zip(ws[keep:], (sp.Float(v, DPS) for v in vals)))
    return xs, us, ws[:keep], [fi.subs(rep) for fi in f], path.subs(rep), final.subs(rep)


def kind_equations(name, kind, lib):
    if kind == "oc":
        return equations(name, lib)
    return equations(name, lib, theta=NOMINAL[name], keep=SYSID_P if kind == "sysid" else 0)


# ---- the product's side -------------------------------------------------------------------------------------------------------------------------------------
def model_gpu(name, kind="oc"):
    """the model through the class surface (PDP.OCSys / PDP.SysID / PDP.ControlPlanning on pdp_amd.sx); .model() generates and compiles it on first use"""
    from pdp_amd import PDP
    from pdp_amd.sx import vertcat
    xs, us, ws, f, path, final = kind_equations(name, kind, "sx")
    label = "fe " + name
    if kind == "oc":
        mdl = PDP.OCSys(label)
        mdl.setAuxvarVariable(vertcat(*ws))
    elif kind == "sysid":
        mdl = PDP.SysID(label)
        mdl.setAuxvarVariable(vertcat(*ws))
    else:
        mdl = PDP.ControlPlanning(label)
    mdl.setStateVariable(vertcat(*xs))
    mdl.setControlVariable(vertcat(*us))
    mdl.setDyn(vertcat(*f))
    if kind != "sysid":
        mdl.setPathCost(path)
        mdl.setFinalCost(final)
    return mdl


def problem(name, kind="oc"):
    from pdp_amd import PDP, codegen
    mdl = model_gpu(name, kind)
    K = {"oc": codegen.KIND_OC, "sysid": codegen.KIND_SYSID, "cp": codegen.KIND_CP}[kind]
    return codegen.Problem(K, mdl.state, mdl.control, mdl.dyn, None if kind == "cp" else mdl.auxvar, None if kind == "sysid" else mdl.path_cost,
                           None if kind == "sysid" else mdl.final_cost, label=PDP._label(mdl.project_name))


@functools.lru_cache(maxsize=None)
def generated(name, kind="oc"):
    """(header source, info) of the code generator - no compiling"""
    from pdp_amd import codegen
    return codegen.generate(problem(name, kind))


def generated_info(name, kind="oc"):
    return generated(name, kind)[1]


LIBRARIES = (("OPS5", "oc"), ("OPS3", "oc"), ("OPT", "oc"), ("OPS5", "sysid"), ("OPS5", "cp"))      # five model libraries in all


# ---- 40-digit references ------------------------------------------------------------------------------------------------------------------------------------
# name of a quantity -> (rows, cols) in terms of n, m, p; what codegen.generate emits as functions and matrix groups
def quantities(kind, n, m, p):
    if kind == "oc":
        return dict(dyn=(n, 1), path_cost=(1, 1), final_cost=(1, 1), costate_step=(n, 1), dhx=(n, 1), dHu=(m, 1), F=(n, n), G=(n, m), E=(n, p), Hxx=(n, n), Hxu=(n, m),
                    Hxe=(n, p), Huu=(m, m), Hue=(m, p), hxx=(n, n), hxe=(n, p), cx=(n, 1))
    if kind == "sysid":
        return dict(dyn=(n, 1), F=(n, n), E=(n, p), G=(n, m))
    return dict(dyn=(n, 1), path_cost=(1, 1), final_cost=(1, 1), dhx=(n, 1), F=(n, n), G=(n, m), cx=(1, n), cu=(1, m))


def _matrices(lib, kind, xs, us, ws, f, path, final):
    """the quantities above as matrices of `lib`, and the costate symbols; derivatives by the library's own differentiation"""
    if lib == "sx":
        from pdp_amd import sx
        x, u, w, lam = sx.vertcat(*xs), sx.vertcat(*us), (sx.vertcat(*ws) if ws else sx.SX()), sx.SX.sym("lam", len(xs))
        jac, col = sx.jacobian, lambda e: sx._lift(e)
        dyn = sx.vertcat(*f)
        dot = lambda: sx.dot(dyn, lam)
        lams = [lam[i] for i in range(len(xs))]
        hess = lambda e, v: sx.hessian(e, v)[0]
    else:
        import sympy as sp
        x, u, w = sp.Matrix(xs), sp.Matrix(us), sp.Matrix(ws)
        lams = list(sp.symbols("lam0:%d" % len(xs), real=True))
        lam = sp.Matrix(lams)
        jac, col = lambda e, v: (sp.Matrix(e).jacobian(v) if len(v) else sp.zeros(len(sp.Matrix(e)), 0)), lambda e: sp.Matrix([e])
        dyn = sp.Matrix(f)
        dot = lambda: (dyn.T * lam)[0, 0]
        hess = lambda e, v: sp.hessian(e, list(v))
    out = dict(dyn=dyn, F=jac(dyn, x), G=jac(dyn, u))
    if kind != "cp":
        out["E"] = jac(dyn, w)
    if kind == "sysid":
        return out, lams
    c, h = col(path), col(final)
    out.update(path_cost=c, final_cost=h, dhx=jac(h, x).T)
    if kind == "cp":
        out.update(cx=jac(c, x), cu=jac(c, u))
        return out, lams
    H = col(path + dot())
    dHx, dHu = jac(H, x).T, jac(H, u).T
    out.update(costate_step=dHx, dHu=dHu, Hxx=jac(dHx, x), Hxu=jac(dHx, u), Hxe=jac(dHx, w), Huu=jac(dHu, u), Hue=jac(dHu, w), hxe=jac(out["dhx"], w), cx=jac(c, x).T)
    out["hxx"] = hess(final, x)                  # through sx.hessian: the one operator of the front-end the code generator does not call
    return out, lams


@functools.lru_cache(maxsize=None)
def _exact_fn(name, kind, final_only=False):
    import sympy as sp
    xs, us, ws, f, path, final = kind_equations(name, kind, "sympy")
    mats, lams = _matrices("sympy", kind, xs, us, ws, f, path, final)
    args = list(xs) + list(us) + lams + list(ws)
    keys = sorted(k for k in mats if not final_only or k in FINAL_KEYS)
    flat = [e for k in keys for e in sp.Matrix(mats[k])]
    fn = sp.lambdify(args, flat, modules="mpmath", cse=True)
    zero = [e == 0 for e in flat]
    return keys, {k: sp.Matrix(mats[k]).shape for k in keys}, fn, zero


FINAL_KEYS = ("final_cost", "dhx", "hxx", "hxe")


def exact(name, kind, x, u, lam, w, final_only=False):
    """every quantity of (name, kind) at one point (final_only: what belongs to the final cost alone), evaluated in 40-digit arithmetic from sympy's derivatives: dict key -> (value rounded to fp64 [r, c], structural-zero
    mask [r, c]).  The arguments are doubles and enter exactly."""
    import mpmath
    keys, shapes, fn, zero = _exact_fn(name, kind, final_only)
    with mpmath.workdps(DPS):
        vals = fn(*[mpmath.mpf(float(v)) for v in list(x) + list(u) + list(lam) + list(w)])
        vals = [float(v) for v in vals]
    out, k0 = {}, 0
    for k in keys:
        r, c = shapes[k]
        out[k] = (np.array(vals[k0:k0 + r * c]).reshape(r, c), np.array(zero[k0:k0 + r * c]).reshape(r, c))
        k0 += r * c
    return out


class Worst:
    """the largest figure per quantity over the cases of one test, and where it occurred; a NaN comes in and stays, whatever follows"""

    def __init__(self):
        self.v = {}

    def add(self, quantity, value, where):
        prev = self.v.get(quantity)
        if prev is None or (prev[0] == prev[0] and not (value <= prev[0])):
            self.v[quantity] = (float(value), where)


def entry_err(got, want, zero):
    """largest |got - want| / |want| over the entries that are not structurally zero; the structural zeros must be exact zeros (else inf)"""
    got, want = np.asarray(got, dtype=float).reshape(want.shape), np.asarray(want, dtype=float)
    if zero.any() and (got[zero] != 0.0).any():
        return float("inf")
    if zero.all():
        return 0.0
    nz = ~zero
    if not np.isfinite(got[nz]).all():
        return float("nan")
    return float((np.abs(got[nz] - want[nz]) / np.abs(want[nz])).max())


# ---- the oracles --------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_oracle(name, kind="oc"):
    import sympy as sp
    from oracle import pdp_oracle as po
    xs, us, ws, f, path, final = kind_equations(name, kind, "sympy")
    if kind == "oc":
        return po.OCSysOracle(sp.Matrix(xs), sp.Matrix(us), list(ws), sp.Matrix(f), path, final)
    if kind == "sysid":
        return po.SysIDOracle(sp.Matrix(xs), sp.Matrix(us), list(ws), sp.Matrix(f))
    return po.ControlPlanningOracle(sp.Matrix(xs), sp.Matrix(us), sp.Matrix(f), path, final)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------------------------
def unit_horizons(name):
    """T = 1, T = 7 and, for OPS5, ROWS + 7 of its fused-unit layout: two backward chunks of unequal length"""
    if name == "OPS3":
        return (1, 7)
    return (1, 7, te.fused3_layout(generated_info(name))["ROWS"] + 7)


def unit_inputs(name, T):
    """the recipe of tile_edge_common.unit_inputs: B = 5, x0 ~ 0.5 N(0, 1), controls ~ 0.3 N(0, 1), standard-normal demonstrations and cotangents, one shared and one
    per-sample parameter (5 % around nominal)"""
    n, m, p = MODELS[name]
    rng = np.random.default_rng(1000 * n + T)
    theta = NOMINAL[name]
    return dict(name=name, B=B, T=T, theta=theta, theta_b=theta[None, :] * (1 + 0.05 * rng.standard_normal((B, p))), x0=0.5 * rng.standard_normal((B, n)),
                u=0.3 * rng.standard_normal((B, T, m)), demo_x=rng.standard_normal((B, T + 1, n)), demo_u=rng.standard_normal((B, T, m)),
                gx=rng.standard_normal((B, T + 1, n)), gu=rng.standard_normal((B, T, m)))


def theta_of(inp, per_sample, b):
    return inp["theta_b"][b] if per_sample else inp["theta"]


@functools.lru_cache(maxsize=None)
def unit_oracle(name, T, per_sample, b):
    """oracle.pdp_oc_unit of sample b - computed once per process, not modified"""
    from oracle import pdp_oracle as po
    inp = unit_inputs(name, T)
    return po.pdp_oc_unit(model_oracle(name), inp["x0"][b], inp["u"][b], theta_of(inp, per_sample, b), inp["demo_x"][b], inp["demo_u"][b])


@functools.lru_cache(maxsize=None)
def unit_exact(name, T, per_sample, b):
    """(X, U) of the same auxiliary system by the reference's formulas in 40-digit arithmetic"""
    from oracle import pdp_oracle as po
    n, m, p = MODELS[name]
    aux = unit_oracle(name, T, per_sample, b)["aux"]
    ex = po.lqr_solver_mp(aux["dynF"], aux["dynG"], aux["dynE"], aux["Hxx"], aux["Huu"], aux["Hxu"], aux["Hxe"], aux["Hue"], aux["hxx"], aux["hxe"], np.zeros((n, p)), T)
    return np.stack(ex["state_traj_opt"]), np.stack(ex["control_traj_opt"])


def in_domain(name, xs, us, w):
    """the smallest margins of a trajectory to the edge of an operator's domain in OPS5 / OPS3: (smallest log / sqrt / pow-base argument, largest |tan argument|,
    largest |exp argument|, largest |tanh argument|) - every argument is bounded away from the edge by construction except through the size of the state"""
    xs, us = np.atleast_2d(xs), np.atleast_2d(us)
    x = lambda i: xs[:, i]
    bases = [1.5 + np.tanh(x(0)), 2.0 + np.sin(x(2 if name == "OPS5" else 1)), np.full(1, w[0] + 1.0), np.full(1, 2.0 + w[1] ** 2), 3.0 + np.cos(us[:, 0])]
    exps = [w[0] * x(2) ** 2, 0.3 * x(1), 0.1 * x(0), np.full(1, w[3])]
    tans = [0.4 * np.tanh(x(1)), 0.2 * x(4 if name == "OPS5" else 2)]
    return dict(base=min(float(b.min()) for b in bases), tan=max(float(np.abs(t).max()) for t in tans), exp=max(float(np.abs(e).max()) for e in exps),
                tanh=float(np.abs(xs).max()))


DOMAIN = dict(base=1e-3, tan=1.4, exp=20.0, tanh=3.0)


def domain_ok(d):
    return d["base"] >= DOMAIN["base"] and d["tan"] <= DOMAIN["tan"] and d["exp"] <= DOMAIN["exp"] and d["tanh"] <= DOMAIN["tanh"]


def opt_points():
    """OPT at T = 1: dict(x0 [B, 16] (the rollout starts here, the matrices are taken here), x1 [B, 16] (given to the kernels that take a trajectory: the final cost's
    argument), u [B, 1, 4], lam [B, 1, 16], theta [12], theta_b [B, 12]).  Inside every domain and away from cancellation: magnitudes in [0.3, 1.3], signs as the rows need"""
    n, m, p = MODELS["OPT"]
    rng = np.random.default_rng(16)
    mag = lambda shape: 0.3 + rng.random(shape)                     # [0.3, 1.3): |tan argument| <= 1.3, exp argument <= 1.3
    sgn = lambda shape: np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    x0 = mag((B, n)) * sgn((B, n))
    for i in (5, 6, 7, 12):                                          # x^0.5; log and x^1.5; sqrt; x^w and x^-0.5: positive
        x0[:, i] = np.abs(x0[:, i])
    for i in (1, 8, 9, 10):                                          # x^3, x^5, x^7, x^-3: negative bases on most rows, one positive
        x0[:, i] = -np.abs(x0[:, i])
        x0[B - 1, i] = -x0[B - 1, i]
    x0[0, 5] = 3.0 - x0[0, 5]                                        # a larger exp argument
    u = mag((B, 1, m)) * sgn((B, 1, m))
    x1 = mag((B, n)) * sgn((B, n))
    lam = mag((B, 1, n)) * sgn((B, 1, n))
    theta = NOMINAL["OPT"]
    return dict(B=B, T=1, x0=x0, x1=x1, u=u, lam=lam, theta=theta, theta_b=theta[None, :] * (1 + 0.05 * rng.standard_normal((B, p))))


# ---- the solver case ------------------------------------------------------------------------------------------------------------------------------------------
def solver_theta():
    th = NOMINAL["OPS5"].copy()
    th[7] = W7_SOLVER
    return th


def solver_x0():
    """two initial states"""
    return 0.8 * np.random.default_rng(5).standard_normal((2, 5))


@functools.lru_cache(maxsize=None)
def solver_oracle(row):
    from oracle import ipopt_ms
    log = []
    ref = ipopt_ms.solve(model_oracle("OPS5"), solver_x0()[row], SOLVER_T, solver_theta(), tol=1e-10, log=log, max_iter=100)
    return ref, log


def rel(a, b):
    return te.rel(a, b)


# ---- OPS5 as SysID --------------------------------------------------------------------------------------------------------------------------------------------
def sysid_horizons():
    """T = 7 and R + 1, R the pool rows of the sweep kernels at this batch size (= the generator's CHUNK up to four trajectories per compute unit)"""
    return (7, generated_info("OPS5", "sysid")["chunk"] + 1)


@functools.lru_cache(maxsize=None)
def sysid_case(T):
    """dict(x0, inputs [B, T, m], theta [5], theta_b [B, 5], xobs [B, T+1, n] (the rollout at the shared theta plus 0.1 N(0, 1), row 0 the initial state), g [B, T+1, n],
    d_theta [B, 5], d_x0 [B, n], d_u [B, T, m]) - shared, not modified"""
    n, m, _ = MODELS["OPS5"]
    p = SYSID_P
    rng = np.random.default_rng(2000 * n + T)
    theta = NOMINAL["OPS5"][:p]
    cs = dict(T=T, theta=theta, theta_b=theta[None, :] * (1 + 0.05 * rng.standard_normal((B, p))), x0=0.5 * rng.standard_normal((B, n)),
              inputs=0.3 * rng.standard_normal((B, T, m)), g=rng.standard_normal((B, T + 1, n)), d_theta=rng.standard_normal((B, p)),
              d_x0=rng.standard_normal((B, n)), d_u=rng.standard_normal((B, T, m)))
    orc = model_oracle("OPS5", "sysid")
    xobs = np.stack([orc.integrateDyn(cs["x0"][b], cs["inputs"][b], theta) for b in range(B)]) + 0.1 * rng.standard_normal((B, T + 1, n))
    xobs[:, 0] = cs["x0"]
    cs["xobs"] = xobs
    return cs


@functools.lru_cache(maxsize=None)
def _sysid_g_fn():
    """G(x, u, theta) = df/du from sympy, from the expressions the oracle is built from (sysid_vjp_u_common.g_fn)"""
    import sympy as sp
    from oracle import pdp_oracle as po
    xs, us, ws, f, _, _ = kind_equations("OPS5", "sysid", "sympy")
    fn = po._lamb([list(xs), list(us), list(ws)], sp.Matrix(f).jacobian(sp.Matrix(us)))
    return lambda x, u, th: np.asarray(fn(x, u, np.asarray(th, float)), float).reshape(len(xs), len(us))


@functools.lru_cache(maxsize=None)
def sysid_reference(T, per_sample, b):
    """sample b by the reference's forward sensitivities: dict(x, F, E, G, X [T+1, n, p] = dx/dtheta, Phi [T+1, n, n] = dx/dx0, D [T, T+1, n, m] = dx_s/du_t, loss, grad,
    gn, grad_theta, grad_x0, grad_u, d_x)"""
    cs = sysid_case(T)
    orc = model_oracle("OPS5", "sysid")
    n, m, p = orc.n, orc.m, orc.p
    th = cs["theta_b"][b] if per_sample else cs["theta"]
    u = cs["inputs"][b]
    x = orc.integrateDyn(cs["x0"][b], u, th)
    aux = orc.getAuxSys(x, u, th)
    F, E = np.stack(aux["dynF"]), np.stack(aux["dynE"])
    G = np.stack([_sysid_g_fn()(x[t], u[t], th) for t in range(T)])
    X = np.stack(orc.integrateAuxSys(aux["dynF"], aux["dynE"], np.zeros((n, p)))["state_traj"])
    Phi = np.stack(orc.integrateAuxSys(aux["dynF"], [np.zeros((n, n))] * T, np.eye(n))["state_traj"])
    D = np.zeros((T, T + 1, n, m))
    for t in range(T):
        D[t, t + 1] = G[t]
        for s in range(t + 2, T + 1):
            D[t, s] = F[s - 1] @ D[t, s - 1]
    dl, g = x - cs["xobs"][b], cs["g"][b]
    return dict(x=x, F=F, E=E, G=G, X=X, Phi=Phi, loss=float((dl * dl).sum()), grad=np.einsum("ti,tip->p", dl, X), gn=np.einsum("tip,tiq->pq", X, X),
                grad_theta=np.einsum("ti,tip->p", g, X), grad_x0=np.einsum("ti,tij->j", g, Phi), grad_u=np.einsum("si,tsij->tj", g, D),
                d_x=X @ cs["d_theta"][b] + Phi @ cs["d_x0"][b] + np.einsum("tsij,tj->si", D, cs["d_u"][b]))


# ---- OPS5 as ControlPlanning ----------------------------------------------------------------------------------------------------------------------------------
CP_PIVOTS = 4
CP_LAYERS = (4, 2)           # a small tanh network: one hidden layer of four units; the output layer included
CP_PATH_NVAR = 25            # variable entries of the `path` group (tests/test_frontend_ops_host.py holds it to the generator's count)
CP_ROWS = min(64, max(4, 2400 // ((CP_PATH_NVAR + 5 + 2 + 16) | 1)))      # ModelLib.cp_vjp_rows' rule, restated


def cp_horizons():
    return (7, CP_ROWS + 1)


def cp_model_gpu(policy, T):
    cp = model_gpu("OPS5", "cp")
    if policy == "poly":
        cp.setPolyControl(np.linspace(0, T, CP_PIVOTS))
    else:
        cp.setNeuralPolicy(list(CP_LAYERS[:-1]))
    return cp


@functools.lru_cache(maxsize=None)
def cp_oracle(policy, T):
    """a ControlPlanningOracle of its own per (policy, T), as cp_vjp_common.oracle_for builds it"""
    import sympy as sp
    from oracle import pdp_oracle as po
    xs, us, _, f, path, final = kind_equations("OPS5", "cp", "sympy")
    orc = po.ControlPlanningOracle(sp.Matrix(xs), sp.Matrix(us), sp.Matrix(f), path, final)
    if policy == "poly":
        orc.setPolyControl(np.linspace(0, T, CP_PIVOTS))
    else:
        orc.setNeuralPolicy(list(CP_LAYERS[:-1]))
    return orc


@functools.lru_cache(maxsize=None)
def cp_case(policy, T):
    """the recipe of cp_edge_common.inputs: x0 ~ 0.5 N(0, 1), theta ~ 0.3 N(0, 1) (Lagrange) or 0.3 / sqrt(max(widths, n)) N(0, 1) (network), one shared and one per
    sample; cotangents and directions standard normal"""
    n, m, _ = MODELS["OPS5"]
    p = cp_oracle(policy, T).n_auxvar
    rng = np.random.default_rng(3000 * n + T + (0 if policy == "poly" else 1))
    theta = (0.3 if policy == "poly" else 0.3 / np.sqrt(max(max(CP_LAYERS), n))) * rng.standard_normal(p)
    return dict(T=T, p=p, theta=theta, theta_b=theta[None, :] * (1 + 0.05 * rng.standard_normal((B, p))), x0=0.5 * rng.standard_normal((B, n)),
                gx=rng.standard_normal((B, T + 1, n)), gu=rng.standard_normal((B, T, m)), d_theta=rng.standard_normal((B, p)), d_x0=rng.standard_normal((B, n)))


@functools.lru_cache(maxsize=None)
def cp_reference(policy, T, per_sample, b):
    """sample b: cp_vjp_common.reference_at (x, u, grad_theta, grad_x0, aux) and beside it cost, step_grad (ControlPlanningOracle.step), dcx, dcu, dhx, d_state, d_control"""
    import cp_vjp_common as cv
    cs, orc = cp_case(policy, T), cp_oracle(policy, T)
    th = cs["theta_b"][b] if per_sample else cs["theta"]
    r = dict(cv.reference_at(orc, cs["x0"][b], T, th, cs["gx"][b], cs["gu"][b]))
    r["cost"], r["step_grad"] = orc.step(cs["x0"][b], T, th)
    x, u = r["x"], r["u"]
    r["dcx"] = np.stack([np.asarray(orc.dcx_fn(x[t], u[t]), float).reshape(-1) for t in range(T)])
    r["dcu"] = np.stack([np.asarray(orc.dcu_fn(x[t], u[t]), float).reshape(-1) for t in range(T)])
    r["dhx"] = np.asarray(orc.dhx_fn(x[-1]), float).reshape(-1)
    X, U, _ = cv.forward_sensitivities(orc, x, u, th)
    v = np.concatenate([cs["d_theta"][b], cs["d_x0"][b]])
    r["d_state"], r["d_control"] = X @ v, U @ v
    return r
