#!/usr/bin/env python3
"""Golden vectors for noisediff_amd.noise_level: the reference's own value-based estimator on the CPU, and sklearn's fit of seeded curves.

    python tests/golden/capture_noise_level.py      # writes tests/golden/noise_level.npz

As in capture_noise_stats.py the functions are taken out of the reference's file with ``ast`` and executed with numpy, torch and sklearn
(1.7.2) in scope: ``get_poisson_lambda``, ``get_poisson_lambda_all_images`` and ``get_regression_result_all_images``
(utils/raw_util.py:248-322).  The reference is repeatable only while it fits at most 141 levels (above that sklearn draws a random subset of
pairs), so every input that goes through it stays within that, and the script asserts it.

Stored: the two frames and the reference's (lambda, sigma); the gap between the reference (fp32 torch.std) and the restatement
(tests/noise_level_ref.py: the integer table, fp64 std), which the tests allow four times over; per fit case of noise_level_ref.FIT_CASES the
restatement's result and the gap between summing the pairs forwards and backwards; sklearn's results for noise_level_ref.SKLEARN_CASES.
For every fitted input the script asserts that no step's squared move lies within a factor 1.01 of tol^2: the stopping test is a branch."""
import ast
import os
import sys
import zipfile

import numpy as np
import sklearn
import torch
from sklearn.linear_model import TheilSenRegressor

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))
from capture_golden import REF as REF_TREE  # noqa: E402  (where the reference checkout is)
import noise_level_ref as R  # noqa: E402

assert sklearn.__version__ == "1.7.2", sklearn.__version__
SEED = 71


def load(path, names, scope):
    tree = ast.parse(open(path).read())
    found = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names}
    assert set(found) == set(names), (path, set(names) - set(found))
    exec(compile(ast.Module(body=list(found.values()), type_ignores=[]), path, "exec"), scope)
    return scope


REF = load(os.path.join(REF_TREE, "utils", "raw_util.py"), {"get_poisson_lambda", "get_poisson_lambda_all_images", "get_regression_result_all_images"},
           {"np": np, "torch": torch, "TheilSenRegressor": TheilSenRegressor})


def clear_of_the_branch(moves, tol, what):
    t2 = tol * tol
    for mv in moves:
        assert not (t2 / 1.01 <= mv <= t2 * 1.01), (what, mv, t2)


out = {"meta.seed": np.int64(SEED)}

# frame A: get_poisson_lambda (the cut at the median keeps it under 141 levels); frame B: the two *_all_images functions, no cut
clean_a, noisy_a = R.level_frame(SEED, (4, 24, 40), 160)
clean_b, noisy_b = R.level_frame(SEED + 1, (4, 16, 20), 120, singleton=False)
for key, clean, noisy, below in (("a", clean_a, noisy_a, True), ("b", clean_b, noisy_b, False)):
    moves = []
    lam, sig, steps, fitted = R.get_poisson_lambda(clean, noisy, below_median=below, moves=moves)
    assert fitted <= 141, fitted
    clear_of_the_branch(moves, 1e-3, key)
    if below:
        ref_lam, ref_sig = REF["get_poisson_lambda"](torch.from_numpy(clean), torch.from_numpy(noisy))
    else:
        d = REF["get_poisson_lambda_all_images"](torch.from_numpy(clean), torch.from_numpy(noisy), {})
        ref_lam, ref_sig = REF["get_regression_result_all_images"](d)
    ref_lam, ref_sig = float(ref_lam), float(ref_sig)
    out[f"{key}.clean"], out[f"{key}.noisy"] = clean, noisy
    out[f"{key}.lambda"], out[f"{key}.sigma"] = np.float64(ref_lam), np.float64(ref_sig)
    out[f"{key}.restated"] = np.array([lam, sig, steps, fitted], np.float64)
    out[f"{key}.gap"] = np.array([abs(lam - ref_lam), abs(sig - ref_sig)], np.float64)
    print(key, "unique", np.unique(clean).size, "fitted", fitted, "reference", ref_lam, ref_sig, "steps", steps, "gap", out[f"{key}.gap"])
assert np.unique(clean_a).size == 163 and int(out["a.restated"][3]) == 81

# the fit cases of the GPU tests: the restatement forwards, and what the order of the sums is worth
for name in R.FIT_CASES:
    x, y, pairs, max_iter, tol = R.fit_case(name)
    moves = []
    slope, icpt, steps = R.theil_sen(x, y, pairs, max_iter, tol, moves=moves)
    if tol > 0:
        clear_of_the_branch(moves, tol, name)
        rev = []
        R.theil_sen(x, y, pairs, max_iter, tol, reverse=True, moves=rev)
        clear_of_the_branch(rev, tol, name)
    out[f"fit.{name}"] = np.array([slope, icpt, steps], np.float64)
    out[f"fit.{name}.gap"] = np.array(R.order_gap(x, y, pairs, max_iter, tol), np.float64)
    print(name, out[f"fit.{name}"], "gap", out[f"fit.{name}.gap"])
levels, xa, ya = R.curve(*[R.stats(R.table(clean_a, noisy_a)[0])[k] for k in (0, 2)])
out["fit.a.gap"] = np.array(R.order_gap(xa, ya), np.float64)

# sklearn itself: all pairs up to 141 points, random_state=0 above
for name, (m, seed, pairs) in R.SKLEARN_CASES.items():
    x, y = R.synthetic_curve(m, seed)
    reg = TheilSenRegressor(random_state=0).fit(x.reshape(-1, 1), y)
    moves = []
    slope, icpt, steps = R.theil_sen(x, y, R.sklearn_pairs(m) if pairs == "sk" else None, moves=moves)
    clear_of_the_branch(moves, 1e-3, name)
    out[f"sklearn.{name}"] = np.array([reg.coef_[0], reg.intercept_, reg.n_iter_ + 1], np.float64)
    print("sklearn", name, out[f"sklearn.{name}"], "restated", slope, icpt, steps, "diff", abs(slope - reg.coef_[0]), abs(icpt - reg.intercept_))
    assert steps == reg.n_iter_ + 1

path = os.path.join(HERE, "noise_level.npz")
with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:      # np.savez_compressed at the highest level
    for k, v in out.items():
        with zf.open(k + ".npy", "w") as f:
            np.lib.format.write_array(f, np.asanyarray(v), allow_pickle=False)
print("bytes", os.path.getsize(path))
assert os.path.getsize(path) < 256 * 1024
