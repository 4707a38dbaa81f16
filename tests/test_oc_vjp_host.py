"""CPU (no GPU needed): the cotangent mode's ABI constant, the autograd module's import, and argument validation of ModelLib.oc_pdp_vjp before any foreign call."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_defines_the_flag_and_keeps_its_33_entry_points():
    src = open(os.path.join(ROOT, "include", "pdp_hip.h")).read()
    assert re.search(r"^#define\s+PDP_OC_COTANGENT\s+8\b", src, flags=re.M)
    flags = {k: int(v) for k, v in re.findall(r"^#define\s+(PDP_OC_[A-Z_]+)\s+(\d+)", src, flags=re.M)}
    assert flags == {"PDP_OC_GIVEN_TRAJ": 1, "PDP_OC_PACKED": 2, "PDP_OC_RECORD_PRIMAL": 4, "PDP_OC_COTANGENT": 8}      # distinct bits
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert len(set(re.findall(r"\b(pdp_[a-z0-9_]+)\s*\(", code))) == 33


def test_autograd_module_imports_without_a_gpu():
    from pdp_amd import autograd
    assert callable(autograd.oc_trajectory)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(TypeError, match="CUDA fp64"):
            autograd.oc_trajectory(None, np.zeros((1, 4)), 5, torch.zeros(7, dtype=torch.float64))


class _NoForeignCalls:
    def __getattr__(self, name):
        raise AssertionError("foreign call %s before the arguments were validated" % name)


def test_runtime_rejects_mismatched_cotangent_shapes_before_any_foreign_call():
    from pdp_amd import runtime
    mdl = runtime.ModelLib.__new__(runtime.ModelLib)
    mdl.n, mdl.m, mdl.p, mdl.lib = 4, 1, 7, _NoForeignCalls()
    B, T = 3, 6
    u, th, x0 = np.zeros((B, T, 1)), np.ones(7), np.zeros((B, 4))
    good_gx, good_gu = np.zeros((B, T + 1, 4)), np.zeros((B, T, 1))
    for gx, gu in ((np.zeros((B, T, 4)), good_gu),              # a cotangent per control step only
                   (good_gx, np.zeros((B, T + 1, 1))),
                   (np.zeros((B, T + 1, 3)), good_gu),
                   (good_gx, np.zeros((B, T, 2))),
                   (np.zeros((B + 1, T + 1, 4)), good_gu),
                   (good_gx[0], good_gu[0])):
        with pytest.raises(ValueError, match="cotangents"):
            mdl.oc_pdp_vjp(u, th, gx, gu, x0=x0)
    with pytest.raises(ValueError, match=r"u must be"):
        mdl.oc_pdp_vjp(np.zeros((B, T, 2)), th, good_gx, good_gu, x0=x0)
    with pytest.raises(ValueError, match="x0"):
        mdl.oc_pdp_vjp(u, th, good_gx, good_gu)
    with pytest.raises(ValueError, match="given trajectory"):
        mdl.oc_pdp_vjp(u, th, good_gx, good_gu, x=np.zeros((B, T + 1, 4)))
    with pytest.raises(ValueError, match="given trajectory"):
        mdl.oc_pdp_vjp(u, th, good_gx, good_gu, x=np.zeros((B, T, 4)), lam=np.zeros((B, T, 4)))
