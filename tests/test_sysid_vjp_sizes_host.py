"""CPU (no GPU needed): the models of tests/test_gpu_sysid_vjp_sizes.py (tests/sysid_vjp_common.py SIZE_MODELS) - dense, wide and 64-state user models of
pdp_sysid_rollout_vjp_batched.  The forward-sensitivity reference against the kernel's recursion in numpy and against central differences, the pool rows (CHUNK) the
generator gives them - the chunk edges of the GPU tests are derived from these - with the register and scratch figures of their sysid_vjp_kernel, and the size refusal
called on a 66-state model."""
import ctypes as C

import numpy as np
import pytest

import sysid_vjp_common as sv

NAME = "pdp_sysid_rollout_vjp_batched"
# what the GPU tests rely on: a pool of 4, 8 and 16 rows (the zoo models and the 40-state chain's siblings have 32 and 16)
CHUNK = {"mlp_6_2_246": 4, "chain_64_4_3": 8, "linear_8_1_64": 16, "linear_8_1_65": 16, "chain_66": 8}
LAUNCHED = [k for k in sorted(sv.SIZE_MODELS) if k != "chain_66"]


def _built(name):
    """(library path, codegen's info) of a SIZE_MODELS entry, compiled for gfx950 once and cached by content hash"""
    import __graft_entry__ as g
    g.build()
    from pdp_amd import codegen
    return codegen.build_problem(sv.size_problem(name)[0])


def horizon(name):
    """the longest horizon the GPU tests run the model at: 3 R + 1 (MLP), 2 R + 1 (chain), R + 1 (linear) with R = CHUNK"""
    return {"mlp_6_2_246": 3, "chain_64_4_3": 2}.get(name, 1) * CHUNK[name] + 1


@pytest.mark.parametrize("name", LAUNCHED)
def test_reference_agrees_with_the_adjoint_recursion_in_numpy(name):
    """forward sensitivities against the costate sweep, both in numpy from the sympy oracle, at the longest horizon of the GPU tests (13 / 17): 1e-13 of the largest
    entry, the bound of tests/test_sysid_vjp_host.py (seen: 4e-16 .. 5e-15)"""
    T = horizon(name)
    c = sv.user_case(name, T=T)
    worst = 0.0
    for b in range(c["inputs"].shape[0]):
        gt, g0 = sv.adjoint_sweep(c["orc"], c["states"][b], c["inputs"][b], c["theta"], c["g"][b])
        worst = max(worst, np.abs(gt - c["grad_theta"][b]).max() / np.abs(gt).max(), np.abs(g0 - c["grad_x0"][b]).max() / np.abs(g0).max())
    print("%s T = %d: forward sensitivities vs adjoint sweep %.2e, max |x| %.2f" % (name, T, worst, np.abs(c["states"]).max()))
    assert worst <= 1e-13


def test_mlp_reference_agrees_with_central_differences_of_the_oracle_rollout():
    """L = sum g . x(theta, x0), sample 0, T = 13: central differences with h = 1e-6 along the parameters at the edges of the four 64-lane slots and along all of x0,
    within 1e-6 of the reference's largest entry (tests/test_sysid_vjp_host.py's step and bound)"""
    c = sv.user_case("mlp_6_2_246", T=horizon("mlp_6_2_246"))
    orc, b, h = c["orc"], 0, 1e-6
    L = lambda v: float((c["g"][b] * orc.integrateDyn(v[orc.p:], c["inputs"][b], v[:orc.p])).sum())
    v0 = np.concatenate([c["theta"], c["x0"][b]])
    ref = np.concatenate([c["grad_theta"][b], c["grad_x0"][b]])
    idx = [0, 63, 64, 191, 192, 245] + list(range(orc.p, orc.p + orc.n))
    fd = np.array([(L(v0 + h * e) - L(v0 - h * e)) / (2 * h) for e in np.eye(v0.size)[idx]])
    et = np.abs(fd[:6] - ref[idx[:6]]).max() / np.abs(c["grad_theta"][b]).max()
    e0 = np.abs(fd[6:] - ref[idx[6:]]).max() / np.abs(c["grad_x0"][b]).max()
    print("mlp_6_2_246: central differences vs the reference: grad_theta %.2e  grad_x0 %.2e" % (et, e0))
    assert et <= 1e-6 and e0 <= 1e-6


@pytest.mark.parametrize("name", sorted(sv.SIZE_MODELS))
def test_pool_rows_and_kernel_resources(name):
    """CHUNK is _pick_chunk's rule on a pool row of the packed (F, E) entries and n cotangents, and has the value the GPU tests' horizons are built around; the figures of
    sysid_vjp_kernel are printed, not bounded: the MLP's and the 64-state chain's instantiations spill"""
    from pdp_amd import codegen
    lib, info = _built(name)
    stride = (info["nvar"]["path"] + info["n"]) | 1
    rule = next((c for c in (32, 16, 8, 4) if c * stride * 8 <= 34 * 1024), 2)
    assert info["chunk"] == codegen._pick_chunk(info["nvar"]["path"], info["n"]) == rule == CHUNK[name]
    kernels = codegen.kernel_resources(lib)
    if name == "chain_66":
        assert "sysid_vjp_kernel" not in kernels                      # the refusal is a compile-time branch: nothing is instantiated
        return
    r = kernels["sysid_vjp_kernel"]
    print("%s: n = %d p = %d path nvar %d CHUNK %d; sysid_vjp_kernel vgpr %d (of them agpr %d) spill %d scratch %d B"
          % (name, info["n"], info["p"], info["nvar"]["path"], info["chunk"], r["vgpr"], r["agpr"], r["spill"], r["scratch"]))
    assert (info["n"], info["p"]) == {"mlp_6_2_246": (6, 246), "chain_64_4_3": (64, 3), "linear_8_1_64": (8, 64), "linear_8_1_65": (8, 65)}[name]


def test_a_66_state_model_is_refused_before_any_launch():
    """PDP_E_SIZE from a SysID model with n = 66, called with valid host pointers and nothing else wrong; PDP_E_ARG comes first; no buffer is touched.  No GPU here: a
    routine that went on to launch would fail with another code"""
    from pdp_amd import runtime as rt
    lib, info = _built("chain_66")
    mdl = rt.load_model(lib)
    assert (mdl.n, mdl.m, mdl.p) == (66, 4, 3)
    keep = [(C.c_double * (5 * 66))() for _ in range(6)]
    for k in keep:
        k[:] = [1.5] * len(k)
    x, u, th, g, gt, g0 = (C.cast(k, C.c_void_p) for k in keep)
    fn = getattr(mdl.lib, NAME)
    assert fn(1, 4, x, u, th, 0, g, gt, g0, None) == -2                           # PDP_E_SIZE
    assert fn(1, 4, x, u, th, 3, g, gt, None, None) == -2 and fn(1, 4, x, u, th, 0, g, None, g0, None) == -2
    assert fn(0, 4, x, u, th, 0, g, gt, g0, None) == -1                           # PDP_E_ARG first
    assert fn(1, 4, x, u, th, 2, g, gt, g0, None) == -1 and fn(1, 4, x, u, th, 0, g, None, None, None) == -1
    assert all(v == 1.5 for k in keep for v in k)
