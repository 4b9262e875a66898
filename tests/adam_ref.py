"""torch.optim.Adam's update restated: the references of tests/test_adam_float64.py.  Nothing here imports noisediff_amd or touches a GPU.

    g' = g + weight_decay p                      (L2 decay added to the gradient, no amsgrad)
    m  = m + (g' - m)(1 - beta1)
    v  = v beta2 + (1 - beta2) g' g'
    p  = p - step_size m / (sqrt(v) / bias2_sqrt + eps),   step_size = lr / (1 - beta1^t),  bias2_sqrt = sqrt(1 - beta2^t)

``step64``    the formula in float64 with the DOUBLE hyper-parameters the caller gave the optimizer.
``step32``    torch.optim.Adam(foreach=False) itself on fp32 CPU tensors with the state injected: the "fp32 reference" of util.derived.
``kernel32``  the arithmetic adam.hip documents, in numpy fp32 with each fma rounded once.  ``complements="double"``: w = float(1 - beta), the complement
              taken in double and rounded once; ``"float"``: w = 1.0f - float(beta), what a kernel that receives the betas as floats can do.
``states`` / ``references``  the one-step tests' cases: sizes, alignments, step counts and magnitude families, shared by the CPU and the GPU tests.

All three take (p, g, m, v) of one tensor BEFORE the step, t = the step count AFTER the increment, and return (p, m, v) after the step.
"""
import functools

import numpy as np
import torch

F32 = np.float32


def step64(p, g, m, v, t, lr, beta1, beta2, eps, weight_decay):
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    beta1, beta2, t = float(beta1), float(beta2), float(t)
    g = g + weight_decay * p
    m = m + (g - m) * (1.0 - beta1)
    v = v * beta2 + (1.0 - beta2) * g * g
    step_size = float(lr) / (1.0 - beta1 ** t)
    bias2_sqrt = np.sqrt(1.0 - beta2 ** t)
    p = p - step_size * (m / (np.sqrt(v) / bias2_sqrt + eps))
    return p, m, v


def torch_adam(p, g, m, v, t, lr, beta1, beta2, eps, weight_decay, dtype):
    """One step of torch.optim.Adam's single-tensor form on CPU tensors of ``dtype`` from the given state (lerp_, mul_().addcmul_(),
    sqrt() / bias2_sqrt + eps, addcdiv_: whatever the installed torch does)."""
    fresh = lambda a: torch.from_numpy(np.array(a)).to(dtype)                      # (np.array copies: the cached states are read-only)
    param = torch.nn.Parameter(fresh(p))
    param.grad = fresh(g)
    opt = torch.optim.Adam([param], lr=float(lr), betas=(float(beta1), float(beta2)), eps=eps, weight_decay=weight_decay, foreach=False)
    opt.state[param] = {"step": torch.tensor(float(t - 1), dtype=torch.float32),
                        "exp_avg": fresh(m), "exp_avg_sq": fresh(v)}
    opt.step()
    st = opt.state[param]
    assert float(st["step"]) == float(t)
    return param.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def step32(p, g, m, v, t, lr, beta1, beta2, eps, weight_decay):
    return torch_adam(p, g, m, v, t, lr, beta1, beta2, eps, weight_decay, torch.float32)


def fma32(a, b, c):
    """a b + c rounded once to fp32 (the product of two fp32 numbers is exact in float64)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def kernel32(p, g, m, v, t, lr, beta1, beta2, eps, weight_decay, complements="double"):
    p, g, m, v = (np.asarray(a, dtype=F32) for a in (p, g, m, v))
    step_size = F32(float(lr) / (1.0 - float(beta1) ** float(t)))                  # the host side, in double
    bias2_sqrt = F32(np.sqrt(1.0 - float(beta2) ** float(t)))
    if complements == "double":
        w1, w2 = F32(1.0 - float(beta1)), F32(1.0 - float(beta2))
    else:
        assert complements == "float"
        w1, w2 = F32(1.0) - F32(beta1), F32(1.0) - F32(beta2)
    b2, eps, wd = F32(beta2), F32(eps), F32(weight_decay)
    g = fma32(wd, p, g)
    m = fma32(g - m, w1, m)
    v = fma32(w2 * g, g, v * b2)
    denom = np.sqrt(v) / bias2_sqrt + eps
    p = p - step_size * (m / denom)
    return p, m, v


# ---------------------------------------------------------------------------------------------------------------- the one-step cases
CHUNK = 8192                                                          # nd_adam_chunk_elements(): the GPU test asserts it
# an empty tail is never launched; these are the smallest sizes that reach a short-only item (1, 7, 8191), a whole vector chunk, a chunk plus one
# element, two whole chunks, and two whole chunks plus a short tail
SIZES = (1, 7, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 5)
MISALIGNED_SIZES = (CHUNK, 2 * CHUNK + 5)                             # vec4 = 0: the whole-chunk scalar path, each of p, g, m, v in turn one float off
STEPS = (1, 2, 10, 1000, 100000)
BETAS = ((0.9, 0.99), (0.9, 0.999))                                   # the reference trainer's, the class default
LR, EPS = 3e-3, 1e-8
# (gradient scale, parameter scale, weight_decay)
FAMILIES = ((1.0, 1.0, 0.0), (1.0, 1e-6, 0.0), (1e-4, 1e-6, 0.0), (1e-8, 1e-6, 0.0), (1.0, 1.0, 0.01), (1e-8, 1.0, 0.01))
TENSORS = ("p", "g", "m", "v")


def layout():
    """[(n, vec4, name of the tensor that starts one float past a 16-byte boundary or None, t)]: 7 aligned items, then 8 with vec4 = 0."""
    items = [(n, 1, None) for n in SIZES] + [(n, 0, off) for n in MISALIGNED_SIZES for off in TENSORS]
    return [(n, vec4, off, STEPS[i % len(STEPS)]) for i, (n, vec4, off) in enumerate(items)]


def zero_grad_indices(n):
    """The fixed handful of elements of a t = 1, weight_decay = 0 item whose gradient is exactly zero."""
    return sorted({0, n // 3, n // 2, n - 1})


@functools.lru_cache(maxsize=None)
def states(family):
    """The state before the step of every item of ``layout()`` for one magnitude family: a tuple of dicts {n, vec4, off, t, p, g, m, v} of fp32
    numpy arrays.  For t = 1: m = v = 0 (and, without weight decay, a handful of zero gradients); otherwise m uniform at the gradient's scale
    and v = u^2 at its square, so v > 0.  Cached: shared, never modified by a caller."""
    gs, ps, wd = FAMILIES[family]
    rng = np.random.default_rng(1000 + family)
    out = []
    for n, vec4, off, t in layout():
        p = (rng.uniform(-1.0, 1.0, n) * ps).astype(F32)
        g = (rng.uniform(-1.0, 1.0, n) * gs).astype(F32)
        if t == 1:
            m, v = np.zeros(n, F32), np.zeros(n, F32)
            if wd == 0.0:
                g[zero_grad_indices(n)] = 0.0
        else:
            m = (rng.uniform(-1.0, 1.0, n) * gs).astype(F32)
            v = ((1.0 - rng.uniform(0.0, 1.0, n)) * gs).astype(F32) ** 2            # u in (0, 1]
        for a in (p, g, m, v):
            a.setflags(write=False)
        out.append(dict(n=n, vec4=vec4, off=off, t=t, p=p, g=g, m=m, v=v))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def references(family, betas, lr):
    """Per item of ``states(family)``: ((p, m, v) of step64, (p, m, v) of step32) at learning rate ``lr`` (a double: LR itself, or the fp32-rounded
    value a capturable kernel can see).  Cached: computed once, shared, never modified."""
    wd = FAMILIES[family][2]
    return tuple((step64(s["p"], s["g"], s["m"], s["v"], s["t"], lr, *betas, EPS, wd), step32(s["p"], s["g"], s["m"], s["v"], s["t"], lr, *betas, EPS, wd))
                 for s in states(family))
