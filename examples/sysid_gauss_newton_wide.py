#!/usr/bin/env python3
"""Gauss-Newton (Levenberg-Marquardt) system identification WITHOUT the Gauss-Newton matrix: pdp_amd.irl.MatrixFreeLM.

The fused SysID.step unit returns G = J'J for models of up to 16 parameters and one loss, "state minus recorded state".  With the rollout's Jacobian-vector product
(SysID.rollout_jvp_batch, include/pdp_hip_sysid_jvp.h) beside its vector-Jacobian product (SysID.rollout_vjp_batch) a product G v costs two launches whatever the
number of parameters and whatever the residual, and the Levenberg-Marquardt step is solved by conjugate gradients on the device.  Two problems:

  1. linear_9_2_99: x+ = x + dt (A x + B u) with all 99 entries of (A, B) unknown, from noise-free rollouts - MatrixFreeLM.for_sysid, the recorded-state residual;
  2. the pendulum of examples/sysid_layer_custom_loss.py (the same recordings): a camera sees the direction of the rod, (sin q, cos q), never the state - a custom
     residual written in torch; length, mass and damping from it, the initial states known.

    python examples/sysid_gauss_newton_wide.py
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pdp_amd import PDP, zoo                        # noqa: E402
from pdp_amd.irl import MatrixFreeLM                # noqa: E402
from pdp_amd.sx import SX, vertcat                  # noqa: E402


def linear_model(n=9, m=2, dt=0.05):
    x, u, a, b = SX.sym("x", n), SX.sym("u", m), SX.sym("a", n * n), SX.sym("b", n * m)
    f = []
    for i in range(n):
        acc = a[i * n] * x[0]
        for j in range(1, n):
            acc = acc + a[i * n + j] * x[j]
        for j in range(m):
            acc = acc + b[i * m + j] * u[j]
        f.append(x[i] + dt * acc)
    sid = PDP.SysID("linear sysid 9 2 99")
    sid.setAuxvarVariable(vertcat(a, b))
    sid.setStateVariable(x)
    sid.setControlVariable(u)
    sid.setDyn(vertcat(*f))
    return sid


def report(name, r, truth):
    print("%s: loss trace %s" % (name, " ".join("%.3e" % v for v in r["loss_trace"])))
    print("%s: %d evaluations, %d rejected, %d CG iterations (2 launches each), stalled %s, parameter error %.3e -> %.3e"
          % (name, r["evaluations"], r["rejected"], r["cg_iterations"], r["stalled"], np.abs(r["parameter_trace"][0] - truth).max(),
             np.abs(r["parameter_trace"][-1] - truth).max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-evals", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)

    sid = linear_model()
    B, T = 16, 20
    truth = 0.5 * rng.standard_normal(99)
    x0, inputs = 0.3 * rng.standard_normal((B, 9)), rng.standard_normal((B, T, 2))
    states = sid.integrateDyn_batch(x0, inputs, truth)
    loop = MatrixFreeLM.for_sysid(sid, inputs, states, truth + 0.1 * rng.standard_normal(99))
    report("linear_9_2_99", loop.run(max_evals=a.max_evals, loss_tol=1e-20), truth)

    env, dt = zoo.make_env("pendulum", "sysid")
    sid = PDP.SysID("pendulum")
    sid.setAuxvarVariable(env.dyn_auxvar)
    sid.setStateVariable(env.X)
    sid.setControlVariable(env.U)
    sid.setDyn(env.X + dt * env.f)
    rng = np.random.default_rng(0)                                                  # (the recordings of examples/sysid_layer_custom_loss.py)
    truth = np.array([1.0, 1.0, 0.05])                                              # l, m, damping_ratio
    B, T = 16, 40
    inputs = torch.as_tensor(rng.uniform(-4.0, 4.0, (B, T, 1)), device="cuda")
    x0 = np.stack([rng.uniform(-1.0, 1.0, B), rng.uniform(-1.0, 1.0, B)], axis=1)
    recorded = sid.integrateDyn_batch(x0, inputs, truth)
    seen = torch.stack([torch.sin(recorded[:, :, 0]), torch.cos(recorded[:, :, 0])], dim=2)
    del recorded

    def residual(state):
        return torch.stack([torch.sin(state[:, :, 0]), torch.cos(state[:, :, 0])], dim=2) - seen

    loop = MatrixFreeLM(sid, x0, inputs, truth * (1.0 + 0.4 * rng.random(3) - 0.2), residual)
    report("pendulum from (sin q, cos q)", loop.run(max_evals=a.max_evals, loss_tol=1e-20), truth)


if __name__ == "__main__":
    main()
