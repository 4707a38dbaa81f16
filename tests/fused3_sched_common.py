"""Shared by tests/test_gpu_fused3_sched.py and probes/record_fused3_sched_golden.py: the inputs of the cases whose outputs tests/golden/fused3_sched_parent.npz records, and
the one function that runs a case.  The golden was written by the recorder on the build of the commit BEFORE the runner's backward step was hand-scheduled
(its hash is in the file): the scheduled kernel issues the same instructions on the same values in another order, so every output must keep every bit.

Quadrotor OC model (n = 13, m = 4, p = 9: oc_pdp_fused3_kernel), B = 3.  The horizons are the edges of the
runner's loops: T = 1, 3 single steps only; 4 exactly one group of U = 4 steps; 5 a group and a single step; 18 two backward chunks (ROWS = 17); 26 two forward chunks
(ROWSF = 25) and the clamp of the gain look-ahead at T - 1."""
import numpy as np

SEED = 20261020
B = 3
N, M = 13, 4
THETA = [1.0, 1.0, 1.0, 1.0, 0.4, 1.0, 1.0, 5.0, 1.0]
HORIZONS = (1, 3, 4, 5, 18, 26)
FIELDS = ("loss", "grad", "x", "lam", "status")
CASES = tuple("T%d" % T for T in HORIZONS) + ("given_T5", "sens_T5", "pivot")
GOLDEN = "fused3_sched_parent.npz"


def quad_inputs(T, seed=SEED):
    """the recipe of the benchmark's batch (random poses, near-hover thrusts, demonstration = hover at the origin) at horizon T"""
    rng = np.random.default_rng(seed + T)
    x0 = np.zeros((B, N))
    x0[:, 0:2] = rng.uniform(-8, 8, (B, 2))
    x0[:, 2] = rng.uniform(5, 10, B)
    ang = rng.uniform(0, 0.5, B)
    axis = rng.standard_normal((B, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    x0[:, 6] = np.cos(ang / 2)
    x0[:, 7:10] = np.sin(ang / 2)[:, None] * axis
    u = 2.5 + 0.3 * rng.standard_normal((B, T, M))
    demo_x = np.zeros((B, T + 1, N))
    demo_x[:, :, 6] = 1.0
    demo_u = np.full((B, T, M), 2.5)
    return x0, u, demo_x, demo_u


def _npy(out, fields):
    return {k: out[k].cpu().numpy().copy() for k in fields}


def run_case(name, given=None):
    """outputs of one case as numpy arrays.  given: (x, lam) of T = 5 for the PDP_OC_GIVEN_TRAJ case - the test hands in the golden's, the recorder its own T5 outputs"""
    if name == "pivot":
        # cheap controls on a rank-one G (tests/riccati_conditioning_common.py): Quu = Huu + G'PG goes from well conditioned (w_u = 1) to far below the guard of the
        # cofactor inverse (w_u = 1e-5) inside one batch, so some steps take the pivoted fallback and drop the reciprocal that was started ahead of the guard's branch
        import riccati_conditioning_common as rc
        n = 6
        mdl, inp = rc.oc_model_gpu(n).model(), rc.oc_inputs(n)
        nb = len(rc.SCALES)
        out = mdl.oc_pdp_grad(inp["u"], inp["theta"], np.zeros((nb, rc.T + 1, n)), np.zeros((nb, rc.T, rc.OC_M)), x0=inp["x0"])
        return _npy(out, FIELDS)
    from pdp_amd import zoo
    mdl = zoo.get("quadrotor", "irl")
    th = np.asarray(THETA)
    if name.startswith("T"):
        x0, u, dx, du = quad_inputs(int(name[1:]))
        return _npy(mdl.oc_pdp_grad(u, th, dx, du, x0=x0), FIELDS)
    x0, u, dx, du = quad_inputs(5)
    if name == "given_T5":
        return _npy(mdl.oc_pdp_grad(u, th, dx, du, x=given[0], lam=given[1]), FIELDS)
    if name == "sens_T5":
        return _npy(mdl.oc_pdp_grad(u, th, dx, du, x0=x0, want_sens=True), FIELDS + ("dxdp", "dudp"))
    raise KeyError(name)
