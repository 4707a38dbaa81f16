#!/usr/bin/env python3
"""Training a feedback policy on a loss ControlPlanning.step cannot express, with the rollout under the policy as a torch.autograd layer.

ControlPlanning.step knows one loss: the model's own path cost and final cost.  Here a tanh-MLP policy u_t = pi(x_t, theta) for the cart-pole is trained, for 16
initial states at once, on a loss written in torch on the output of pdp_amd.autograd.cp_trajectory: the pole angle at T/2 and the full state at T towards given values,
plus a small effort term on the controls.  `loss.backward()` is one launch of the adjoint sweep (cp_vjp_kernel): the sensitivities
dx_t/dtheta are never formed.  torch.optim.Adam moves the parameters.

    python examples/cp_layer_custom_loss.py --iters 200 --lr 1e-2
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
from pdp_amd.autograd import cp_trajectory       # noqa: E402

ANGLE = 1                                        # cart-pole state: (x, q, dx, dq)


def custom_loss(state, control, angle_mid, final_state, effort):
    T = control.shape[1]
    return ((state[:, T // 2, ANGLE] - angle_mid) ** 2).sum() + ((state[:, T] - final_state) ** 2).sum() + effort * (control ** 2).sum()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--horizon", type=int, default=30)
    ap.add_argument("--hidden", type=int, nargs="*", default=[8, 8])
    ap.add_argument("--effort", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)

    env, dt = zoo.make_env("cartpole", "oc")
    cp = PDP.ControlPlanning("cartpole")           # (same label and equations as the pre-built zoo model: no compilation at run time)
    cp.setStateVariable(env.X)
    cp.setControlVariable(env.U)
    cp.setDyn(env.X + dt * env.f)
    cp.setPathCost(env.path_cost)                  # (the layer does not use the model's cost; the class asks for one)
    cp.setFinalCost(env.final_cost)
    cp.setNeuralPolicy(a.hidden)

    B, T = a.batch, a.horizon
    f64 = dict(dtype=torch.float64, device="cuda")
    rng = np.random.default_rng(a.seed)
    x0 = np.zeros((B, 4))
    x0[:, 0], x0[:, 1] = rng.uniform(-0.3, 0.3, B), rng.uniform(-0.4, 0.4, B)
    ini = torch.tensor(x0, **f64)
    angle_mid = torch.full((B,), 0.1, **f64)                               # the pole angle half way
    final_state = torch.zeros((B, 4), **f64)                               # upright and at rest at the origin at T
    theta = torch.tensor(0.1 * rng.standard_normal(cp.n_auxvar), requires_grad=True, **f64)       # one policy for all initial states
    opt = torch.optim.Adam([theta], lr=a.lr)
    loss_trace = []
    torch.cuda.synchronize()
    t0 = time.time()
    for k in range(a.iters):
        if k == a.iters // 2:                                              # (the first iterations load code objects and build the optimiser's state)
            torch.cuda.synchronize()
            t_half = time.time()
        opt.zero_grad()
        state, control = cp_trajectory(cp, ini, T, theta)
        loss = custom_loss(state, control, angle_mid, final_state, a.effort)
        loss.backward()                                                    # theta.grad = dL/dtheta, summed over the 16 rollouts
        opt.step()
        loss_trace.append(float(loss.detach()))
        if k % max(1, a.iters // 10) == 0 or k == a.iters - 1:
            print("iter %5d  loss %.6e" % (k, loss_trace[-1]))
    torch.cuda.synchronize()
    t1 = time.time()
    print("done: %d Adam steps x %d rollouts of %d steps, p = %d, in %.2f s, %.2f ms per step over the second half  (loss %.4e -> %.4e)"
          % (a.iters, B, T, cp.n_auxvar, t1 - t0, 1e3 * (t1 - t_half) / (a.iters - a.iters // 2), loss_trace[0], loss_trace[-1]))
    return loss_trace


if __name__ == "__main__":
    main()
