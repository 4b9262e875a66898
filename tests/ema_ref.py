"""The shadow-model update restated in fp64 numpy: the reference of tests/test_ema.py.  ema_pytorch's rule (EMA.update / get_current_decay /
update_moving_average) written out from its definition -- nothing here imports the package or noisediff_amd.

    s = step before the call, step becomes s + 1 in every case
    s % update_every != 0                skip
    s <= update_after_step               copy
    not initted                          copy, initted = True, then lerp (a no-op in value)
    otherwise                            lerp with weight 1 - decay
    e = max(s + 1 - update_after_step - 1, 0);  decay = 0 if e <= 0 else clamp(1 - (1 + e / inv_gamma) ** -power, min_value, beta)
"""
import numpy as np

SKIP, COPY, LERP, COPY_LERP = 0, 1, 2, 3


def decay(s, beta, update_after_step, inv_gamma=1.0, power=2.0 / 3.0, min_value=0.0):
    """The decay of the call that finds the counter at ``s`` (the package evaluates it after the increment), in fp64."""
    e = max(np.float64(s) + 1.0 - update_after_step - 1.0, 0.0)
    if e <= 0.0:
        return 0.0
    value = 1.0 - np.power(1.0 + e / np.float64(inv_gamma), -np.float64(power))
    return float(min(max(value, np.float64(min_value)), np.float64(beta)))


def plan(s, initted, beta, update_after_step, update_every, inv_gamma=1.0, power=2.0 / 3.0, min_value=0.0):
    """-> (action, weight in fp64, initted after the call)."""
    if s % update_every != 0:
        return SKIP, 0.0, initted
    if s <= update_after_step:
        return COPY, 0.0, initted
    return (LERP if initted else COPY_LERP), 1.0 - decay(s, beta, update_after_step, inv_gamma, power, min_value), True


def weight32(w):
    """The fp64 weight rounded to fp32 once, as the pass applies it."""
    return float(np.float32(w))


def lerp(ema, src, w):
    """torch.lerp's form in fp64."""
    ema, src = np.asarray(ema, np.float64), np.asarray(src, np.float64)
    return ema + w * (src - ema) if w < 0.5 else src - (src - ema) * (1.0 - w)


class Shadow:
    """The whole state: {name: fp64 array}, step, initted.  ``update(online)`` applies one call with the online tensors of that moment; the lerp uses
    the weight rounded to fp32 (the one rounding the contract allows) on fp64 values."""

    def __init__(self, tensors, beta, update_after_step, update_every, inv_gamma=1.0, power=2.0 / 3.0, min_value=0.0, no_ema=()):
        self.t = {k: np.array(v, dtype=np.float64) for k, v in tensors.items()}
        self.args = (beta, update_after_step, update_every, inv_gamma, power, min_value)
        self.no_ema, self.step, self.initted = set(no_ema), 0, False

    def update(self, online):
        action, w, self.initted = plan(self.step, self.initted, *self.args)
        self.step += 1
        if action != SKIP:
            for k, src in online.items():
                src = np.asarray(src, np.float64)
                if action in (COPY, COPY_LERP) or k in self.no_ema:
                    self.t[k] = src.copy()
                if action in (LERP, COPY_LERP) and k not in self.no_ema:
                    self.t[k] = lerp(self.t[k], src, weight32(w))
        return action, w
