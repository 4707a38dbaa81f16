#!/usr/bin/env python3
"""Planning to a reference trajectory is least squares: Gauss-Newton (Levenberg-Marquardt) on a policy WITHOUT the Gauss-Newton matrix, beside Adam on the same problem.

A Lagrange-polynomial policy u_t = sum_i b_i(t) U_i for the cart-pole, one theta = vcat(U_0 .. U_N) shared by 16 initial states, is fitted to a reference the policy can
reach exactly: the rollouts under a hidden theta*.  The residual - written in torch on (state, control) - is state minus reference.

  1. pdp_amd.irl.MatrixFreeLM.for_cp: one rollout per evaluation; every conjugate-gradient iteration of a step is J v (the tangent sweep, cp_jvp_kernel,
     ControlPlanning.rollout_jvp_batch) followed by J' w (the adjoint sweep, cp_vjp_kernel, ControlPlanning.rollout_vjp_batch) on the SAVED rollout - two launches
     whatever the number of parameters;
  2. torch.optim.Adam through pdp_amd.autograd.cp_trajectory on the same loss from the same start: one rollout and one adjoint sweep per step.

Printed: evaluations (rollouts), CG iterations and the losses of both.  Measured, not asserted.

    python examples/cp_gauss_newton_plan.py
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pdp_amd import PDP, zoo                     # noqa: E402
from pdp_amd.autograd import cp_trajectory       # noqa: E402
from pdp_amd.irl import MatrixFreeLM             # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--horizon", type=int, default=30)
    ap.add_argument("--pivots", type=int, default=8)
    ap.add_argument("--max-evals", type=int, default=30)
    ap.add_argument("--adam-iters", type=int, default=200)
    ap.add_argument("--lr", type=float, default=5e-2)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)

    env, dt = zoo.make_env("cartpole", "oc")
    cp = PDP.ControlPlanning("cartpole")           # (same label and equations as the pre-built zoo model: no compilation at run time)
    cp.setStateVariable(env.X)
    cp.setControlVariable(env.U)
    cp.setDyn(env.X + dt * env.f)
    cp.setPathCost(env.path_cost)                  # (neither loop uses the model's cost; the class asks for one)
    cp.setFinalCost(env.final_cost)
    cp.setPolyControl(np.linspace(0, a.horizon, a.pivots))

    B, T, p = a.batch, a.horizon, cp.n_auxvar
    rng = np.random.default_rng(a.seed)
    x0 = np.zeros((B, 4))
    x0[:, 0], x0[:, 1] = rng.uniform(-0.3, 0.3, B), rng.uniform(-0.4, 0.4, B)
    hidden = 2.0 * rng.standard_normal(p)          # theta*: the reference is reachable, the floor of the loss is rounding
    start = hidden + 1.0 * rng.standard_normal(p)
    reference = cp.integrateSys_batch(x0, T, hidden)[0]

    def residual(state, control):
        return state - reference

    loop = MatrixFreeLM.for_cp(cp, x0, T, start, residual)
    r = loop.run(max_evals=a.max_evals, loss_tol=1e-22)
    print("Levenberg-Marquardt, matrix-free: loss trace %s" % " ".join("%.3e" % v for v in r["loss_trace"]))
    print("Levenberg-Marquardt, matrix-free: %d evaluations (rollouts), %d rejected, %d CG iterations (2 sweeps each), stalled %s, |theta - theta*| %.3e -> %.3e"
          % (r["evaluations"], r["rejected"], r["cg_iterations"], r["stalled"], np.abs(r["parameter_trace"][0] - hidden).max(),
             np.abs(r["parameter_trace"][-1] - hidden).max()))

    ini = torch.tensor(x0, dtype=torch.float64, device="cuda")
    theta = torch.tensor(start, dtype=torch.float64, device="cuda", requires_grad=True)
    opt = torch.optim.Adam([theta], lr=a.lr)
    adam = []
    for _ in range(a.adam_iters):
        opt.zero_grad()
        state, control = cp_trajectory(cp, ini, T, theta)
        loss = (residual(state, control) ** 2).sum() / B
        loss.backward()
        opt.step()
        adam.append(float(loss.detach()))
    print("Adam through cp_trajectory (lr %g): %d steps = %d rollouts + %d adjoint sweeps, loss %.3e -> %.3e, |theta - theta*| %.3e"
          % (a.lr, a.adam_iters, a.adam_iters, a.adam_iters, adam[0], adam[-1], float((theta.detach().cpu() - torch.as_tensor(hidden)).abs().max())))
    return dict(lm=r, adam=np.array(adam))


if __name__ == "__main__":
    main()
