#!/usr/bin/env python3
"""Fitting the INITIAL STATES of optimal control solves, with the OC solution as a torch.autograd layer that is differentiable in its initial state.

The initial state is the input of an MPC layer: a state estimator or an encoder in front of the controller trains through dL/dx_0.  Here the smallest such problem:
the cart-pole at a FIXED parameter theta, 16 solves, and the question "from which initial states does the optimal trajectory pass through given values at T/2 and
at T?".  The targets are the states at T/2 and T of the solves from hidden initial states; the fit starts from perturbed ones.  The loss is written in torch on the
output of pdp_amd.autograd.oc_trajectory(..., ini_grad=True); `loss.backward()` differentiates through the OC solution - one launch of the fused unit in its
cotangent mode and, behind it, the adjoint sweep that gives dL/dx_0 (pdp_oc_sens_out.grad_x0) - and a torch.optim optimiser moves the initial states.

    python examples/oc_layer_initial_state.py --iters 60 --lr 2e-2
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pdp_amd import PDP, zoo                     # noqa: E402
from pdp_amd.autograd import oc_trajectory       # noqa: E402
from pdp_amd.sx import vertcat                   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--lr", type=float, default=2e-2)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--sigma", type=float, default=0.2, help="initial guess = hidden initial state + N(0, sigma^2)")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    env, dt = zoo.make_env("cartpole", "irl")
    oc = PDP.OCSys("cartpole")
    oc.setAuxvarVariable(vertcat(env.dyn_auxvar, env.cost_auxvar))
    oc.setControlVariable(env.U)
    oc.setStateVariable(env.X)
    oc.setDyn(env.X + dt * env.f)
    oc.setPathCost(env.path_cost)
    oc.setFinalCost(env.final_cost)

    B, T = a.batch, a.horizon
    f64 = dict(dtype=torch.float64, device="cuda")
    rng = np.random.default_rng(a.seed)
    theta = torch.tensor([0.5, 0.5, 1.0, 1.0, 6.0, 1.0, 1.0], **f64)              # fixed: it requires no gradient
    hidden = np.zeros((B, 4))
    hidden[:, 0], hidden[:, 1] = rng.uniform(-0.3, 0.3, B), rng.uniform(-0.5, 0.5, B)
    frames = [T // 2, T]
    with torch.no_grad():
        target = oc_trajectory(oc, torch.tensor(hidden, **f64), T, theta, ini_grad=True)[0][:, frames].clone()
    ini = torch.tensor(hidden + a.sigma * rng.standard_normal(hidden.shape), requires_grad=True, **f64)
    opt = torch.optim.Adam([ini], lr=a.lr)
    loss_trace, warm = [], None
    t0 = time.time()
    for k in range(a.iters):
        opt.zero_grad()
        state, control, info = oc_trajectory(oc, ini, T, theta, return_info=True, ini_grad=True, warm_start=warm)
        warm = {key: info[key] for key in ("state", "control", "costate")}         # the next solve starts from this one
        loss = ((state[:, frames] - target) ** 2).sum()
        loss.backward()                                                             # ini.grad = dL/dx_0 through the OC solution
        opt.step()
        loss_trace.append(float(loss))
        print("iter %5d  loss %.6e  |x0 - hidden x0| %.4f" % (k, loss_trace[-1], float(np.abs(ini.detach().cpu().numpy() - hidden).max())))
    print("done: %d iterations x %d solves of %d steps, states at T/2 and T as targets, in %.2f s  (loss %.4e -> %.4e)"
          % (a.iters, B, T, time.time() - t0, loss_trace[0], loss_trace[-1]))
    return loss_trace


if __name__ == "__main__":
    main()
