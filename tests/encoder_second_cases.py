"""Shared by tests/test_encoder_second_order_abi.py and tests/test_gpu_encoder_second_order.py: the float64 pure-PyTorch statements of the
frequency and the SH encoder (differentiated by autograd, never by hand), and the shapes of the second-order tests."""
import functools
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BATCHES = (1, 64, 65, 257, 1000)          # a single lane, a full wave, wave + 1, block + 1, a ragged tail
FREQ_SHAPES = ((3, 4), (3, 10), (2, 6), (1, 1), (3, 0))   # (D, deg)
SH_DEGREES = tuple(range(1, 9))


def freq_reference(x, deg):
    """cat([x, sin(2^f x), cos(2^f x) ...]) on a [B, D] tensor, in its dtype"""
    cols = [x]
    for f in range(deg):
        cols += [torch.sin(x * 2.0 ** f), torch.cos(x * 2.0 ** f)]
    return torch.cat(cols, -1)


def gen_sh():
    tools = os.path.join(ROOT, 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import gen_sh as module
    return module


@functools.lru_cache(maxsize=None)
def sh_functions():
    """the 64 basis polynomials of tools/gen_sh.py as Python callables of (x, y, z): sympy.lambdify, plain arithmetic on whatever it is given"""
    import sympy as sp
    g = gen_sh()
    return tuple(sp.lambdify((g.x, g.y, g.z), e, modules='math') for e in g.basis())


def sh_reference(p, degree):
    """[B, degree^2] from a [B, 3] tensor, in its dtype (a constant polynomial is broadcast)"""
    x, y, z = p.unbind(-1)
    cols = [f(x, y, z) for f in sh_functions()[:degree * degree]]
    return torch.stack([c if torch.is_tensor(c) else torch.full_like(x, float(c)) for c in cols], -1)


def unit_vectors(n, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, 3, generator=g, dtype=torch.float64)
    return (v / v.norm(dim=-1, keepdim=True)).to(dtype)


def three_orders(fn, x, w, v):
    """y = fn(x); gx = d (w . y) / dx (create_graph); then d (v . gx) / dw and d (v . gx) / dx.  x, w leaves that require grad.
    Returns y, gx, dL/dw, dL/dx (zeros where autograd reports no dependence)."""
    y = fn(x)
    (gx,) = torch.autograd.grad(y, x, w, create_graph=True)
    if not gx.requires_grad:
        return y.detach(), gx.detach(), torch.zeros_like(w), torch.zeros_like(x)
    dw, dx = torch.autograd.grad(gx, (w, x), v, allow_unused=True)
    return y.detach(), gx.detach(), torch.zeros_like(w) if dw is None else dw, torch.zeros_like(x) if dx is None else dx


EPS32 = math.ldexp(1.0, -23)
