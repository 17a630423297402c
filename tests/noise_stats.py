"""Statistics helpers of the noise tests: moment checks at 5 sigma and chi-square goodness of fit
against the exact normal / Poisson laws.  tests/test_noise_cpu.py runs them on torch's own CPU
``randn`` and ``poisson`` first, so the yardstick is pinned on the reference sampler before it judges
a kernel.  All inputs are 1-D float arrays (numpy or torch); the arithmetic is fp64 numpy."""
import math

import numpy as np


def _np(v):
    return v.detach().cpu().double().numpy() if hasattr(v, "detach") else np.asarray(v, dtype=np.float64)


def chi2_cap(dof):
    """The acceptance bound dof + 6 sqrt(2 dof): six standard deviations of a chi-square variable."""
    return dof + 6.0 * math.sqrt(2.0 * dof)


def corr(a, b):
    a, b = _np(a), _np(b)
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


def normal_checks(n, pair=None, max_abs=None, bins=64):
    """dict name -> (value, bound) for standard-normal draws ``n``: |mean| <= 5 / sqrt(N), |var - 1| <=
    5 sqrt(2 / N), lag-1 correlation <= 5 / sqrt(N), the correlation with ``pair`` (the second
    Box-Muller output) <= 5 / sqrt(N), max |n| <= max_abs, chi-square over ``bins`` equiprobable bins."""
    from statistics import NormalDist
    n = _np(n)
    N = n.size
    out = {"mean": (abs(n.mean()), 5 / math.sqrt(N)), "var": (abs(n.var() - 1.0), 5 * math.sqrt(2.0 / N)),
           "lag1": (abs(corr(n[:-1], n[1:])), 5 / math.sqrt(N))}
    if pair is not None:
        out["pair"] = (abs(corr(n, pair)), 5 / math.sqrt(N))
    if max_abs is not None:
        out["max_abs"] = (float(np.abs(n).max()), max_abs)
    edges = np.array([NormalDist().inv_cdf(k / bins) for k in range(1, bins)])
    counts = np.bincount(np.searchsorted(edges, n), minlength=bins)
    exp = N / bins
    out["chi2"] = (float(((counts - exp) ** 2 / exp).sum()), chi2_cap(bins - 1))
    return out


def poisson_pmf(lam, kmax):
    k = np.arange(kmax + 1)
    return np.exp(-lam + k * math.log(lam) - np.array([math.lgamma(i + 1.0) for i in k]))


def poisson_checks(s, lam, min_expected=20.0):
    """dict name -> (value, bound) for Poisson(lam) draws ``s``: mean within 5 sqrt(lam / N), variance
    within 5 sqrt((lam + 2 lam^2) / N), every value a non-negative integer ("integer": violations, 0),
    chi-square against the exact pmf with the cells of expected count < min_expected pooled into the
    two tails."""
    s = _np(s)
    N = s.size
    out = {"integer": (float(((s < 0) | (s != np.floor(s)) | ~np.isfinite(s)).sum()), 0.0),
           "mean": (abs(s.mean() - lam), 5 * math.sqrt(lam / N)),
           "var": (abs(s.var() - lam), 5 * math.sqrt((lam + 2 * lam * lam) / N))}
    kmax = int(lam + 12 * math.sqrt(lam) + 40)
    exp = N * poisson_pmf(lam, kmax)
    ok = np.nonzero(exp >= min_expected)[0]
    lo, hi = int(ok[0]), int(ok[-1])  # the pmf is unimodal: the kept cells are one run
    k = np.clip(np.nan_to_num(s, nan=0.0), 0, kmax + 1).astype(np.int64)
    counts = np.bincount(k, minlength=kmax + 2).astype(np.float64)
    cells_obs, cells_exp = list(counts[lo:hi + 1]), list(exp[lo:hi + 1])
    if lo > 0:  # lower tail: k < lo
        cells_obs.insert(0, counts[:lo].sum())
        cells_exp.insert(0, exp[:lo].sum())
    cells_obs.append(counts[hi + 1:].sum())  # upper tail: k > hi, exact mass by complement
    cells_exp.append(N - exp[:hi + 1].sum())
    o, e = np.array(cells_obs), np.array(cells_exp)
    keep = e > 0
    if not keep.all():
        assert o[~keep].sum() == 0, "draws in a cell of zero mass"
    o, e = o[keep], e[keep]
    out["chi2"] = (float(((o - e) ** 2 / e).sum()), chi2_cap(len(e) - 1))
    return out


def poisson_pair_checks(a, b, lam):
    """dict name -> (value, bound) for two Poisson(lam) samples that should be independent (two
    streams of one state): their correlation <= 5 / sqrt(N), and the fraction of positions where
    they are equal within 5 sigma of its law -- each position is equal with probability
    p = sum_k pmf(k)^2, so the fraction is binomial with standard deviation sqrt(p (1 - p) / N).
    Shared draws (one stream rereading another's words) raise both."""
    a, b = _np(a), _np(b)
    N = a.size
    pmf = poisson_pmf(lam, int(lam + 12 * math.sqrt(lam) + 40))
    p = float((pmf * pmf).sum())
    return {"corr": (abs(corr(a, b)), 5 / math.sqrt(N)),
            "equal": (abs(float((a == b).mean()) - p), 5 * math.sqrt(p * (1 - p) / N))}


def failures(checks):
    return {k: v for k, v in checks.items() if not v[0] <= v[1]}
