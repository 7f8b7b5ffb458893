"""wsl_adam_step against torch.optim.Adam (CPU, float32) and a float64 restatement (tests/dan_ref.py): five consecutive steps of the
DAN trainer's setting (lr 1e-4, betas (0.9, 0.99), eps 1e-8) over arenas that straddle the vector width, with gradients of 0 and of
1e-12 (where eps decides the update) and with grad_scale.

Criterion: every UPDATE p_t - p_(t-1) within 1e-4 of lr of the float64 one (an Adam update is at most ~lr in size, so this is the
1e-4-of-scale criterion of the other op tests; comparing parameters would hide any error behind their size)."""
import numpy as np
import pytest
import torch

import dan_ref as R

LR, BETAS, EPS = 1e-4, (0.9, 0.99), 1e-8


@pytest.mark.parametrize("gs", [1.0, 0.5])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4099])
def test_adam_five_steps(be, n, gs):
    rng = np.random.default_rng(n * 7 + int(gs * 10))
    # parameters of size 1e-3: storing p in float32 rounds each update by up to ulp(p) / 2 = 6e-8 |p|, which at |p| ~ 1 would be six
    # times the bound; at 1e-3 it is 6e-11 and the comparison sees the update's arithmetic, which is what it is about
    p0 = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    grads = [(rng.standard_normal(n) * 10.0 ** rng.integers(-4, 1, n)).astype(np.float32) for _ in range(5)]
    for g in grads:
        g[0] = 0.0
        if n > 1:
            g[1] = 1e-12
    # ---- torch.optim.Adam in float32, and the float64 restatement, on the scaled gradient
    pt = torch.from_numpy(p0.copy()).requires_grad_()
    opt = torch.optim.Adam([pt], lr=LR, betas=BETAS, eps=EPS)
    p64 = torch.from_numpy(p0).double()
    m64, v64 = torch.zeros_like(p64), torch.zeros_like(p64)
    # ---- device
    p, m, v = be.arr(p0), be.zeros((n,)), be.zeros((n,))
    prev, prev64, prev_t = p0.astype(np.float64), p64.clone(), p0.copy()
    worst = 0.0
    for step, g in enumerate(grads, 1):
        gd = be.arr(g)
        be.call("wsl_adam_step", be.ptr(p), be.ptr(gd), be.ptr(m), be.ptr(v), n, LR, BETAS[0], BETAS[1], EPS, step, gs, be.stream)
        be.sync()
        pt.grad = torch.from_numpy(g * np.float32(gs))
        opt.step()
        R.adam_step(p64, torch.from_numpy(g).double() * gs, m64, v64, step, LR, BETAS, EPS)
        got = be.np(p).astype(np.float64)
        upd, upd64 = got - prev, (p64 - prev64).numpy()
        upd_t = pt.detach().numpy().astype(np.float64) - prev_t
        err = float(np.max(np.abs(upd - upd64)))
        worst = max(worst, err)
        assert err <= 1e-4 * LR, (step, err)
        assert float(np.max(np.abs(upd - upd_t))) <= 1e-4 * LR, step
        assert upd[0] == 0.0                                 # zero gradient from zero state: no movement
        prev, prev64, prev_t = got, p64.clone(), pt.detach().numpy().copy()
    print(f"adam n={n} gs={gs}: worst update error {worst:.3e} (bound {1e-4 * LR:.1e})")


def test_adam_refusals(be):
    p = be.zeros((4,))
    assert be.lib.wsl_adam_step(None, be.ptr(p), be.ptr(p), be.ptr(p), 4, LR, 0.9, 0.99, EPS, 1, 1.0, be.stream) == -1
    assert be.lib.wsl_adam_step(be.ptr(p), be.ptr(p), be.ptr(p), be.ptr(p), 4, LR, 0.9, 0.99, EPS, 0, 1.0, be.stream) == -1
    assert be.lib.wsl_adam_step(be.ptr(p), be.ptr(p), be.ptr(p), be.ptr(p), 0, LR, 0.9, 0.99, EPS, 1, 1.0, be.stream) == -1
