"""Shared by tests/test_cp_edge_inputs.py (CPU) and tests/test_gpu_cp_edge.py (GPU, in-process and in its child processes): the ControlPlanning.step kernels on three
user models at the far end of the sizes their tuned route advertises (n <= 16, m <= 4), the policies that reach every kernel of that route, their inputs, the host's
routing rules restated, and a second formulation of the gradient in 40-digit arithmetic.

    name   n  m   the chain of tests/tile_edge_common.py it is     what it reaches
    C16   16  4   E16                                              no padding row in any state tile, layer 0 of a network fills all 16 lanes, M = 4
    C15   15  3   E15                                              the odd size next to the full tile
    C5     5  1   E5                                               the first size past the small-system algebra, one control

ControlPlanning has no auxvar: theta_nominal(name) of the chain is substituted as numbers (tile_edge_common.equations(.., theta=..)) in both symbolic libraries.
Product: PDP.ControlPlanning on pdp_amd.sx.  Oracle: oracle.pdp_oracle.ControlPlanningOracle on sympy (forward sensitivities, the reference's order).

Policies.  Lagrange: pivots linspace(0, T, N), p = N m, sensitivity tiles of 16 parameters.  tanh MLP: `layers` includes the output layer.  POLY and MLP below list every
case with its horizons; route() says which kernel family the host hands it to (restated from csrc/pdp_model.hip and csrc/pdp_cp_mlp_kernels.h), the environment of the
child process (tests/test_gpu_cp_edge.py) which kernel of that family.

Inputs: B = 5, default_rng(1000 n + T): x0 ~ 0.5 N(0, 1), theta ~ 0.3 N(0, 1) (Lagrange) or 0.3 / sqrt(max(widths, n)) N(0, 1) (MLP), one shared theta and one per sample
(5 % around the shared one).

Parameter blocks: a gradient is compared block by block, each relative to the largest entry of ITS block - the 16-column tiles of the Lagrange policy, each vec(A_k) and
each b_k of a network.  Relative to the largest entry of the whole gradient, a 1e-10 bound leaves 1e-6 of the smallest block of the eight-layer case unchecked (its largest
entry is 9.8e-5 of the gradient's), which is room for a wrong tile or layer block."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import tile_edge_common as te  # noqa: E402

MODELS = {"C16": (16, 4), "C15": (15, 3), "C5": (5, 1)}
CHAIN = {"C16": "E16", "C15": "E15", "C5": "E5"}
NAMES = sorted(MODELS)
B_UNIT = 5
REF_CAP = te.REF_CAP          # the oracle's own fp64 error against 40 digits stays below this
TOL_LOSS = 1e-11              # BASELINE.md section 3 / tests/test_gpu_generic_sizes.py: the project's fp64 tolerances
TOL = 1e-10
CHUNK = 32                    # what the code generator reports for all three (tests/test_cp_edge_inputs.py)

HORIZONS = (1, 7, 32, 33, 65)        # at N = 6: one step; inside a chunk; one full chunk; two chunks of 17 + 16; three chunks and more than 64 steps for the lane-strided loops
TILE_HORIZONS = (7, 33)
# (model, pivots) -> horizons
POLY = {(name, 6): HORIZONS for name in NAMES}
POLY.update({("C16", 4): TILE_HORIZONS,           # p = 16: one full tile
             ("C16", 5): TILE_HORIZONS,           # p = 20: the last tile has 4 columns
             ("C16", 12): TILE_HORIZONS,          # p = 48
             ("C16", 16): TILE_HORIZONS + (65,),  # p = 64: NT = 4, the maximum
             ("C15", 5): TILE_HORIZONS,           # p = 15
             ("C15", 16): TILE_HORIZONS,          # p = 48          (("C15", 6), p = 18, is above: one pivot's controls straddle the tile boundary)
             ("C5", 1): TILE_HORIZONS,            # p = 1
             ("C5", 16): TILE_HORIZONS})          # p = 16
MAX_PIVOTS = 16               # N = 17 is PDP_E_ARG
MLP_HORIZONS = (1, 7, 65)     # pool rows are <= 64 in every layout: T = 65 forces a second evaluation pass
# (model, layers) -> (route, p or None)
MLP = {("C16", (4,)): ("register", 68),                          # one layer
       ("C16", (16, 4)): ("register", 340),                      # a full 16 x 16 layer
       ("C16", (12, 16, 4)): ("register", 480),                  # non-square hidden layers
       ("C16", (8, 8, 8, 4)): ("register", 316),                 # four layers
       ("C15", (16, 8, 8, 3)): ("register", 491),                # four layers, odd n
       ("C5", (1,)): ("register", 6),                            # one layer, m = 1
       ("C5", (16, 16, 1)): ("register", 385),                   # width 16 at n = 5
       ("C16", (20, 4)): ("adjoint", 424),                       # width 17 - 32
       ("C5", (32, 1)): ("adjoint", 225),                        # MLP_MAX_WIDTH
       ("C5", (6,) * 7 + (1,)): ("adjoint", 295),                # eight layers
       ("C16", (16, 16, 4)): ("generic", 612),                   # p > 512
       ("C5", (33, 1)): ("generic", None),                       # width beyond 32
       ("C5", (6,) * 8 + (1,)): ("generic", None)}               # nine layers
OFFLOAD_CASE = ("C16", (12, 16, 4), 65)      # the adjoint kernel with its activations in the workspace: from offload_batch(.., cus) trajectories on
CLASS_MLP = {"C16": (12, 16, 4), "C15": (16, 8, 8, 3), "C5": (16, 16, 1)}      # the class-surface test: N = 6 and this network, T = 7
CLASS_T = 7
PAIR_T = 7                    # the workgroup shapes of the pair kernel: each model at its largest tile count
PAIR_PIVOTS = {name: max(N for (nm, N) in POLY if nm == name) for name in NAMES}


def poly_cases(name=None):
    return [(nm, N, T) for (nm, N), Ts in sorted(POLY.items()) if name in (None, nm) for T in Ts]


def mlp_cases(name=None, routes=("register", "adjoint", "generic")):
    return [(nm, layers, T) for (nm, layers), (r, _) in sorted(MLP.items()) if name in (None, nm) and r in routes for T in MLP_HORIZONS]


# ---- the models -------------------------------------------------------------------------------------------------------------------------------------------
def model_gpu(name):
    """PDP.ControlPlanning on the product's symbolic engine; .model() generates and compiles it on first use"""
    from pdp_amd import PDP
    from pdp_amd.sx import vertcat
    xs, us, _, f, path, final = te.equations(CHAIN[name], "sx", theta=te.theta_nominal(CHAIN[name]))
    cp = PDP.ControlPlanning("cp edge " + name)
    cp.setStateVariable(vertcat(*xs))
    cp.setControlVariable(vertcat(*us))
    cp.setDyn(vertcat(*f))
    cp.setPathCost(path)
    cp.setFinalCost(final)
    return cp


def problem(name):
    from pdp_amd import PDP, codegen
    cp = model_gpu(name)
    return codegen.Problem(codegen.KIND_CP, cp.state, cp.control, cp.dyn, None, cp.path_cost, cp.final_cost, label=PDP._label(cp.project_name))


@functools.lru_cache(maxsize=None)
def generated_info(name):
    """what the code generator says of the model - no compiling"""
    from pdp_amd import codegen
    return codegen.generate(problem(name))[1]


@functools.lru_cache(maxsize=None)
def _sympy_equations(name):
    return te.equations(CHAIN[name], "sympy", theta=te.theta_nominal(CHAIN[name]))


def model_oracle(name):
    """a fresh ControlPlanningOracle of the same equations (the policy is set on it by the caller)"""
    import sympy as sp
    from oracle import pdp_oracle as po
    xs, us, _, f, path, final = _sympy_equations(name)
    return po.ControlPlanningOracle(sp.Matrix(xs), sp.Matrix(us), sp.Matrix(f), path, final)


@functools.lru_cache(maxsize=None)
def _oracle_with(name, kind, key, T):
    orc = model_oracle(name)
    if kind == "poly":
        orc.setPolyControl(np.linspace(0, T, key))
    else:
        orc.setNeuralPolicy(list(key[:-1]))
    return orc


# ---- the host's routing rules, restated (csrc/pdp_model.hip cp_step / cp_needs_generic / mlp_shape / cp_prepass_ws_bytes, csrc/pdp_cp_mlp_kernels.h cp_mlp16_ok,
#      csrc/pdp_model_kernels.h cp_adjoint_layout / cp_adjoint_plan, csrc/pdp_launch.h traj_per_workgroup / split_tiles) -------------------------------------------
MLP_MAX_WIDTH, MLP_MAX_LAYERS, MLP16_W, MLP16_MAXL, CP_MAX_P = 32, 8, 16, 4, 512
traj_per_workgroup = te.traj_per_workgroup


def mlp_params(n, layers):
    sizes = [n] + list(layers)
    return sum(sizes[k + 1] * sizes[k] + sizes[k + 1] for k in range(len(layers)))


def cp_mlp16_ok(n, m, layers):
    return 1 <= len(layers) <= MLP16_MAXL and n <= MLP16_W and m <= MLP16_W and all(1 <= w <= MLP16_W for w in layers)


def cp_needs_generic(n, m, layers=None, p=0):
    """layers None: the Lagrange policy"""
    if n > 16 or m > 4:
        return True
    return layers is not None and (p > CP_MAX_P or len(layers) > MLP_MAX_LAYERS or max(layers) > MLP_MAX_WIDTH)


def route(name, layers):
    n, m = MODELS[name]
    if cp_needs_generic(n, m, layers, mlp_params(n, layers)):
        return "generic"
    return "register" if cp_mlp16_ok(n, m, layers) else "adjoint"


def tiles(p):
    return (p + 15) // 16


def chunks(T):
    """lengths of the sensitivity kernels' chunks: ceil(T / CHUNK) chunks of ceil(T / nchunk) steps, the last one short"""
    nchunk = -(-T // CHUNK)
    ch = -(-T // nchunk)
    return [min(ch, T - k * ch) for k in range(nchunk)]


def split_tiles(nt, want):
    gy = 1 if want < 1 else min(nt, want)
    per = -(-nt // gy)
    return -(-nt // per), per


def cp_pair_slice(info, T, pivots):
    """doubles of LDS per trajectory of cp_step_poly2_kernel (csrc/pdp_cp_pair_kernels.h); the host takes the pair kernel while slice x trajectories per workgroup fits 160 KB"""
    n, m = info["n"], info["m"]
    d = 1 + info["nconst"]["path"] + info["chunk"] * (info["nvar"]["path"] | 1) + (T + 1) * n + T * m + T * pivots + n + 8 + 64 + max(n, m) + 8
    return (d + 1) & ~1


def prepass_ws_bytes(name, B, T):
    n, m = MODELS[name]
    return B * ((T + 1) * n + T * m + n) * 8


def cp_adjoint_layout_total(info, layers, p, T, offload, rows):
    n, m = info["n"], info["m"]
    actw = sum(layers[:-1]) if layers is not None else 0
    o = p + (T + 1) * n + (0 if offload else T * actw) + (8 * MLP_MAX_WIDTH + 1) + 8 * MLP_MAX_WIDTH + n + (m + n)
    o += 1 + info["nconst"]["path"] + rows * (info["nvar"]["path"] | 1)
    return o + 8


def cp_adjoint_plan(info, layers, p, T, B, cus, have_ws=True):
    """(offload, rows)"""
    stride = info["nvar"]["path"] | 1
    rows = 64 if 64 * stride * 8 <= 34 * 1024 else info["chunk"]
    resident = cp_adjoint_layout_total(info, layers, p, T, False, rows) * 8
    if not have_ws or layers is None or resident <= 40 * 1024:
        return False, rows
    if B <= cus * (160 * 1024 // resident):
        return False, rows
    fit = (40 * 1024 // 8 - cp_adjoint_layout_total(info, layers, p, T, True, 0)) // stride
    if fit < 8:
        return False, rows
    return True, min(fit, 64)


def offload_batch(cus):
    """the smallest batch whose adjoint kernel offloads its activations for OFFLOAD_CASE on a device of `cus` compute units (0: it never does)"""
    name, layers, T = OFFLOAD_CASE
    info = generated_info(name)
    p = mlp_params(MODELS[name][0], layers)
    if not cp_adjoint_plan(info, layers, p, T, 1 << 30, cus)[0]:
        return 0
    resident = cp_adjoint_layout_total(info, layers, p, T, False, cp_adjoint_plan(info, layers, p, T, 1, cus)[1]) * 8
    return cus * (160 * 1024 // resident) + 1


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------------------
def n_params(name, kind, key):
    n, m = MODELS[name]
    return key * m if kind == "poly" else mlp_params(n, key)


def inputs(name, kind, key, T):
    """kind "poly": key = number of pivots; "mlp": key = layers (tuple).  dict(B, T, p, x0 [B, n], theta [p], theta_b [B, p])"""
    n, m = MODELS[name]
    rng = np.random.default_rng(1000 * n + T)
    p = n_params(name, kind, key)
    x0 = 0.5 * rng.standard_normal((B_UNIT, n))
    scale = 0.3 if kind == "poly" else 0.3 / np.sqrt(max(max(key), n))
    theta = scale * rng.standard_normal(p)
    return dict(name=name, B=B_UNIT, T=T, p=p, x0=x0, theta=theta, theta_b=theta[None, :] * (1 + 0.05 * rng.standard_normal((B_UNIT, p))))


def big_rows(name, kind, key, T, B):
    """x0 [B, n] of the large batches: the five base initial states, repeated with a 1 % perturbation (default_rng(B)); theta is the shared one"""
    inp = inputs(name, kind, key, T)
    x0 = inp["x0"][np.arange(B) % B_UNIT] * (1 + 0.01 * np.random.default_rng(B).standard_normal((B, MODELS[name][0])))
    x0[:B_UNIT] = inp["x0"]
    return x0


def theta_of(inp, per_sample, b):
    return inp["theta_b"][b] if per_sample else inp["theta"]


def blocks(name, kind, key):
    """[(label, lo, hi)] - the parameter blocks a gradient is judged by"""
    n, m = MODELS[name]
    if kind == "poly":
        p = key * m
        return [("tile %d" % k, 16 * k, min(16 * k + 16, p)) for k in range(tiles(p))]
    out, o, cols = [], 0, n
    for k, rows in enumerate(key):
        out.append(("A%d" % k, o, o + rows * cols))
        o += rows * cols
        out.append(("b%d" % k, o, o + rows))
        o += rows
        cols = rows
    return out


def block_rel(a, b, blks):
    """max over the blocks of max|a - b| / max|b| within the block"""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return max(float(np.abs(a[lo:hi] - b[lo:hi]).max() / np.abs(b[lo:hi]).max()) for _, lo, hi in blks)


rel = te.rel


@functools.lru_cache(maxsize=None)
def oracle_step(name, kind, key, T, per_sample, b):
    """dict(loss, grad, x, u) of ControlPlanningOracle on sample b - once per process, not modified"""
    inp = inputs(name, kind, key, T)
    return oracle_step_at(name, kind, key, T, inp["x0"][b], theta_of(inp, per_sample, b))


def oracle_step_at(name, kind, key, T, x0, theta):
    orc = _oracle_with(name, kind, key, T)
    loss, grad = orc.step(x0, T, theta)
    sol = orc.integrateSys(x0, T, theta)
    return dict(loss=loss, grad=grad, x=sol["state_traj"], u=sol["control_traj"])


# ---- the same step in 40-digit arithmetic, by the costate recursion (the kernels' adjoint formulation; the oracle propagates forward sensitivities):
#      mu_T = h_x;   v_t = c_u + G_t' mu_{t+1};   grad += (d pi/d theta)' v_t;   mu_t = c_x + F_t' mu_{t+1} + (d pi/d x)' v_t -----------------------------------
@functools.lru_cache(maxsize=None)
def _mp_functions(name):
    import sympy as sp
    xs, us, _, f, path, final = _sympy_equations(name)
    F, c, h = sp.Matrix(f), sp.Matrix([path]), sp.Matrix([final])
    lam = lambda e, args=(xs, us): sp.lambdify(list(args), e, modules="mpmath")
    return dict(f=lam(F), fx=lam(F.jacobian(xs)), fu=lam(F.jacobian(us)), c=lam(c), cx=lam(c.jacobian(xs)), cu=lam(c.jacobian(us)), h=lam(h, (xs,)), hx=lam(h.jacobian(xs), (xs,)))


def exact_step(name, kind, key, T, x0, theta, dps=40):
    """(loss, grad [p]) as floats rounded from `dps`-digit values, on the exact doubles of x0 and theta"""
    import mpmath as mp
    n, m = MODELS[name]
    fn = _mp_functions(name)
    with mp.workdps(dps):
        th = [mp.mpf(float(v)) for v in theta]
        p = len(th)
        x = [mp.mpf(float(v)) for v in x0]
        if kind == "poly":
            piv = [mp.mpf(float(v)) for v in np.linspace(0, T, key)]

            def basis(t):
                out = []
                for i in range(key):
                    bi = mp.mpf(1)
                    for j in range(key):
                        if j != i:
                            bi = bi * (t - piv[j]) / (piv[i] - piv[j])
                    out.append(bi)
                return out
        else:
            shapes, o, cols = [], 0, n
            for rows in key:
                shapes.append((o, rows, cols))          # A_k at o (column-major), b_k behind it
                o += rows * cols + rows
                cols = rows
        xs, us, keep = [x], [], []
        loss = mp.mpf(0)
        for t in range(T):
            if kind == "poly":
                bt = basis(t)
                u = [sum(bt[i] * th[i * m + j] for i in range(key)) for j in range(m)]
                keep.append(bt)
            else:
                z, zs = x, []
                for k, (o, rows, cols) in enumerate(shapes):
                    if k > 0:
                        z = [mp.tanh(a) for a in z]
                    zs.append(z)
                    z = [sum(th[o + r + c * rows] * z[c] for c in range(cols)) + th[o + rows * cols + r] for r in range(rows)]
                u = z
                keep.append(zs)
            loss += fn["c"](x, u)[0]
            us.append(u)
            x = list(fn["f"](x, u))
            xs.append(x)
        loss += fn["h"](x)[0]
        mu = list(fn["hx"](x))
        grad = [mp.mpf(0)] * p
        for t in range(T - 1, -1, -1):
            x, u = xs[t], us[t]
            Fx, Fu, cx, cu = fn["fx"](x, u), fn["fu"](x, u), fn["cx"](x, u), fn["cu"](x, u)
            v = [cu[j] + sum(Fu[i, j] * mu[i] for i in range(n)) for j in range(m)]
            dpx = [mp.mpf(0)] * n
            if kind == "poly":
                bt = keep[t]
                for i in range(key):
                    for j in range(m):
                        grad[i * m + j] += bt[i] * v[j]
            else:
                delta = v
                for k in range(len(shapes) - 1, -1, -1):
                    o, rows, cols = shapes[k]
                    z = keep[t][k]
                    for c in range(cols):
                        for r in range(rows):
                            grad[o + r + c * rows] += delta[r] * z[c]
                    for r in range(rows):
                        grad[o + rows * cols + r] += delta[r]
                    dz = [sum(th[o + r + c * rows] * delta[r] for r in range(rows)) for c in range(cols)]
                    delta = [dz[c] * (1 - z[c] * z[c]) for c in range(cols)] if k > 0 else dz          # z_k = tanh(a_{k-1})
                dpx = delta
            mu = [cx[i] + sum(Fx[r, i] * mu[r] for r in range(n)) + dpx[i] for i in range(n)]
        return float(loss), np.array([float(g) for g in grad])
