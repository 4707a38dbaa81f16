"""CPU: the conditions under which tests/test_gpu_cp_edge.py means something, checked on the oracle, the code generator and the compiler alone (no GPU).

1. Sizes and routes: the three models of tests/cp_edge_common.py have the (n, m) they are there for and CHUNK = 32; every case has the parameter count and the tile
   count it is listed for, and the host's routing rules, restated, hand it to the kernel family it is meant for (register kernels, the adjoint kernel's own range, the
   size-generic kernel); the batch of the offloaded adjoint route does offload under the restated cp_adjoint_plan (769 trajectories at 256 compute units) and B = 5 does not.
2. Reference accuracy: for every case at its longest horizon - sample 0 with the shared theta and the last sample with its own - ControlPlanningOracle.step (forward
   sensitivities, fp64) against the costate recursion in 40-digit arithmetic on the same doubles: loss <= 1e-12 relative, gradient <= 1e-12 of the largest entry OF EACH
   BLOCK, no gradient entry exactly zero.  Measured: loss <= 1.5e-15; gradient <= 4.2e-15 per block on the tuned route, 1.3e-14 for nine layers and 4.7e-14 for width 33
   (the two deepest / widest networks, which go to the size-generic kernel); no zeros; the smallest block maximum over the overall maximum is 9.8e-5 for the eight-layer
   network and 2.6e-5 for the nine-layer one.  The measured values are printed.
3. Register record: the three libraries are compiled and every cp_* kernel's VGPRs, AGPRs, spills and scratch are printed; none spills vector registers."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import cp_edge_common as c  # noqa: E402

CUS = 256                     # compute units of an MI355X: the restated rules are checked at this count (the GPU test takes the device's own)


@pytest.mark.parametrize("name", c.NAMES)
def test_sizes_and_chunk(name):
    info = c.generated_info(name)
    assert (info["n"], info["m"], info["p"]) == c.MODELS[name] + (0,)
    assert info["chunk"] == c.CHUNK == 32
    n, m = c.MODELS[name]
    assert not c.cp_needs_generic(n, m) and c.cp_needs_generic(17, m) and c.cp_needs_generic(n, 5)
    assert {"C16": n == 16 and m == 4, "C15": n == 15 and m == 3, "C5": n == 5 and m == 1}[name]


def test_polynomial_cases_reach_the_tiles_and_chunks_they_name():
    p = {(nm, N): N * c.MODELS[nm][1] for nm, N in c.POLY}
    assert [p[k] for k in (("C16", 4), ("C16", 5), ("C16", 12), ("C16", 16), ("C15", 5), ("C15", 6), ("C15", 16), ("C5", 1), ("C5", 16))] == [16, 20, 48, 64, 15, 18, 48, 1, 16]
    assert [c.tiles(v) for v in (1, 15, 16, 18, 20, 48, 64)] == [1, 1, 1, 2, 2, 3, 4] and c.tiles(17 * 4) == 5
    assert p["C16", 5] % 16 == 4                                                        # the last tile has four columns
    assert 16 % c.MODELS["C15"][1] != 0                                                 # a pivot's controls straddle the boundary between tiles 0 and 1
    assert max(p.values()) == 64 and all(N <= c.MAX_PIVOTS for _, N in c.POLY)          # p <= 64: the forward-sensitivity kernels, not the adjoint kernel
    for (nm, N), Ts in c.POLY.items():
        assert set(c.TILE_HORIZONS) <= set(Ts)
    assert c.POLY["C16", 16] == (7, 33, 65) and all(c.POLY[nm, 6] == (1, 7, 32, 33, 65) for nm in c.NAMES)
    # chunks of equal length (cp_step_poly_kernel: nchunk = ceil(T / CHUNK), ch = ceil(T / nchunk))
    assert [c.chunks(T) for T in c.HORIZONS] == [[1], [7], [32], [17, 16], [22, 22, 21]]
    # which instantiation a batch reaches: at B = 5 the one-wave kernel spreads its tiles over grid.y, at B = 2 CUs + 1 one workgroup carries them all; the pair kernel
    # carries them all from B = CUs + 1 on
    assert c.split_tiles(4, 4 * CUS // 5) == (4, 1) and c.split_tiles(4, 4 * CUS // (2 * CUS + 1)) == (1, 4) and c.split_tiles(3, 2 * CUS // (CUS + 1)) == (1, 3)
    assert [c.traj_per_workgroup(B, CUS) for B in (5, CUS, CUS + 1, 2 * CUS, 2 * CUS + 1)] == [1, 1, 2, 2, 4]
    assert c.PAIR_PIVOTS == {"C16": 16, "C15": 16, "C5": 16}
    # the pair kernel is taken (PDP_CP_POLY_VARIANT=3) while its LDS slices fit a CU: every case at one trajectory per workgroup, the large batches at two and four
    for nm, N, T in c.poly_cases():
        assert c.cp_pair_slice(c.generated_info(nm), T, N) * 8 <= 160 * 1024, (nm, N, T)
    for nm in c.NAMES:
        assert c.cp_pair_slice(c.generated_info(nm), c.PAIR_T, c.PAIR_PIVOTS[nm]) * 4 * 8 <= 160 * 1024, nm


def test_network_cases_reach_the_kernels_they_name():
    for (nm, layers), (want, p) in c.MLP.items():
        n, m = c.MODELS[nm]
        assert layers[-1] == m
        assert c.route(nm, layers) == want, (nm, layers)
        if p is not None:
            assert c.mlp_params(n, layers) == p, (nm, layers)
        assert len(c.blocks(nm, "mlp", layers)) == 2 * len(layers) and c.blocks(nm, "mlp", layers)[-1][2] == c.mlp_params(n, layers)
    reg = [k for k, v in c.MLP.items() if v[0] == "register"]
    assert {len(l) for _, l in reg} == {1, 2, 3, 4} and any(16 in l[:-1] for _, l in reg) and any(len(set(l[:-1])) > 1 for _, l in reg)
    adj = [l for (_, l), v in c.MLP.items() if v[0] == "adjoint"]
    assert any(len(l) == c.MLP_MAX_LAYERS for l in adj) and any(max(l) == c.MLP_MAX_WIDTH for l in adj) and any(16 < max(l) < 32 for l in adj)
    gen = [(nm, l) for (nm, l), v in c.MLP.items() if v[0] == "generic"]
    assert any(c.mlp_params(c.MODELS[nm][0], l) > c.CP_MAX_P and c.cp_mlp16_ok(*c.MODELS[nm], l) for nm, l in gen)      # p > 512 alone hands a register-kernel shape over
    assert any(max(l) == c.MLP_MAX_WIDTH + 1 for _, l in gen) and any(len(l) == c.MLP_MAX_LAYERS + 1 for _, l in gen)
    # pool rows <= 64 in every layout: T = 65 takes a second evaluation pass
    for (nm, layers), (want, _) in c.MLP.items():
        if want != "generic":
            info = c.generated_info(nm)
            assert c.cp_adjoint_plan(info, layers, c.mlp_params(c.MODELS[nm][0], layers), 65, c.B_UNIT, CUS) == (False, 64), (nm, layers)
    assert max(c.MLP_HORIZONS) == 65


def test_offloaded_adjoint_route_is_reached():
    name, layers, T = c.OFFLOAD_CASE
    info = c.generated_info(name)
    p = c.mlp_params(c.MODELS[name][0], layers)
    B = c.offload_batch(CUS)
    assert B == 769
    assert c.cp_adjoint_plan(info, layers, p, T, B, CUS)[0] and not c.cp_adjoint_plan(info, layers, p, T, B - 1, CUS)[0] and not c.cp_adjoint_plan(info, layers, p, T, c.B_UNIT, CUS)[0]
    assert not c.cp_adjoint_plan(info, layers, p, T, B, CUS, have_ws=False)[0]
    offload, rows = c.cp_adjoint_plan(info, layers, p, T, B, CUS)
    assert 8 <= rows <= 64 and c.cp_adjoint_layout_total(info, layers, p, T, True, rows) * 8 <= 40 * 1024 < c.cp_adjoint_layout_total(info, layers, p, T, False, 64) * 8


def _reference_cases():
    out = [(nm, "poly", N, max(Ts)) for (nm, N), Ts in sorted(c.POLY.items())]
    return out + [(nm, "mlp", layers, max(c.MLP_HORIZONS)) for (nm, layers) in sorted(c.MLP)]


@pytest.mark.parametrize("case", _reference_cases(), ids=lambda k: "%s-%s-%s-T%d" % (k[0], k[1], "x".join(map(str, k[2])) if k[1] == "mlp" else k[2], k[3]))
def test_oracle_is_accurate_on_the_inputs(case):
    name, kind, key, T = case
    inp = c.inputs(name, kind, key, T)
    blks = c.blocks(name, kind, key)
    for per_sample, b in ((False, 0), (True, c.B_UNIT - 1)):
        o = c.oracle_step(name, kind, key, T, per_sample, b)
        loss, grad = c.exact_step(name, kind, key, T, inp["x0"][b], c.theta_of(inp, per_sample, b))
        el, eg = abs(o["loss"] - loss) / abs(loss), c.block_rel(o["grad"], grad, blks)
        small = min(np.abs(grad[lo:hi]).max() for _, lo, hi in blks) / np.abs(grad).max()
        print("%s %s %s T=%d %s theta sample %d: oracle vs 40 digits: loss %.2e, gradient per block %.2e; %d zero entries; smallest block maximum / overall maximum %.2e"
              % (name, kind, key, T, "per-sample" if per_sample else "shared", b, el, eg, int((grad == 0).sum()) + int((o["grad"] == 0).sum()), small))
        assert el <= c.REF_CAP and eg <= c.REF_CAP, (case, per_sample, b, el, eg)
        assert (grad != 0).all() and (o["grad"] != 0).all(), (case, per_sample, b)


def test_register_record_of_the_cp_kernels():
    """compiled side by side (content-hash cache of codegen.build_problem; hipcc takes 14 s for C5, about a minute for C16 on first use).  Measured: no kernel spills;
    cp_step_mlp4t_kernel<4> of C16 uses 440 registers, 184 of them AGPRs; cp_auxsys_kernel has 4752 B of scratch without spills (local arrays indexed by the policy description)"""
    from concurrent.futures import ThreadPoolExecutor
    from pdp_amd import codegen
    with ThreadPoolExecutor(max_workers=3) as ex:
        libs = dict(zip(c.NAMES, ex.map(lambda nm: codegen.build_problem(c.problem(nm))[0], c.NAMES)))
    wanted = {"cp_step_poly_kernel", "cp_step_poly2_kernel", "cp_poly_rollout_lanes_kernel", "cp_step_mlp16_kernel", "cp_step_mlp4t_kernel", "cp_step_adjoint_kernel",
              "cp_integrate_kernel", "cp_auxsys_kernel", "cp_step_generic_kernel"}
    for name in c.NAMES:
        res = {k: v for k, v in codegen.kernel_resources(libs[name]).items() if k.startswith("cp_")}
        assert wanted <= {k.split("<")[0] for k in res}, (name, sorted(res))
        for k in sorted(res):
            r = res[k]
            print("%s %s: %d VGPRs, %d AGPRs, %d spilled, %d B of scratch" % (name, k, r["vgpr"], r["agpr"], r["spill"], r["scratch"]))
        for k, r in res.items():
            assert r["spill"] == 0, (name, k, r)
