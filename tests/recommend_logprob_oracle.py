"""The float64 oracle of recommend(sample_temperature=, return_logprob=True) (include/arx_sample_logp.h): given a
row's scores, which columns are eligible, the temperature and the picks in selection order, the log-probability of every
pick under the Plackett-Luce law over the row's eligible columns -- and the tolerance a float32 evaluation is held to."""
import numpy as np

import tags_oracle as T


def eligible(L, tags=None, want_any=None, want_all=None, ex_lists=None):
    """bool [B, V]: not excluded, passes the tag test, score > -inf (ELIGIBLE of the header)."""
    return T.masked(L, tags, want_any, want_all, ex_lists) > -np.inf


def _lse(a):
    if len(a) == 0:
        return -np.inf
    m = a.max()
    return m + np.log(np.exp(a - m).sum())


def logp(L, elig, picks, tau):
    """float64 [B, k]: logp[r][t] = a_t - log sum over REST u {pick t .. last} of exp(a), a = L[r] / tau[r]; 0 for a
    tau == 0 row and for a -1 column."""
    picks = np.asarray(picks)
    B, k = picks.shape
    out = np.zeros((B, k), dtype=np.float64)
    for r in range(B):
        if tau[r] == 0:
            continue
        a = L[r].astype(np.float64) / np.float64(tau[r])
        pk = picks[r][picks[r] >= 0]
        assert len(set(pk.tolist())) == len(pk) and elig[r][pk].all(), "row %d: picks must be distinct and eligible" % r
        assert (picks[r][:len(pk)] >= 0).all(), "row %d: -1 entries come last" % r
        rest = elig[r].copy()
        rest[pk] = False
        run = _lse(a[rest])
        for t in range(len(pk) - 1, -1, -1):
            run = np.logaddexp(run, a[pk[t]])
            out[r, t] = a[pk[t]] - run
    return out


def tolerance(L, elig, tau, lp):
    """[B, k]: 2^-20 (1 + (smax - smin) / tau) + 2^-22 |logp| + n_eligible 2^-24 per row (the slate sampler's bound with C
    read as the row's eligible count); tau == 0 rows: 0 (their logp is exactly 0)."""
    B = L.shape[0]
    out = np.zeros_like(lp)
    for r in range(B):
        if tau[r] == 0 or not elig[r].any():
            continue
        s = L[r][elig[r]].astype(np.float64)
        out[r] = 2.0 ** -20 * (1 + (s.max() - s.min()) / np.float64(tau[r])) + 2.0 ** -22 * np.abs(lp[r]) \
            + elig[r].sum() * 2.0 ** -24
    return out


def worst(got, exp, tol):
    """the largest |error| / tolerance over the entries with a tolerance; entries of tolerance 0 must be exact"""
    zero = tol == 0
    assert (got[zero] == exp[zero]).all()
    if zero.all():
        return 0.0
    return float((np.abs(got.astype(np.float64) - exp)[~zero] / tol[~zero]).max())


def draw(L, elig, tau, seed, k):
    """The float64 restatement's own draw: int64 [B, k], the k eligible columns of largest key
    float32(float64(tau) * g + s) by (key desc, column asc), g the float64 noise of (seed, row, column)
    (sample_oracle: bits, gumbel64) -- the sampled recommend of arx_sample.h; -1 past the last eligible column."""
    import sample_oracle as SM
    import slate_sample_oracle as SS
    L = np.asarray(L, dtype=np.float32)
    B, V = L.shape
    out = np.full((B, k), -1, dtype=np.int64)
    cols = np.arange(V)
    for r in range(B):
        g = SM.gumbel64(SM.bits(seed, [r], cols.astype(np.uint32)))[0]
        img = SS.image(SS.keys(L[r], g, float(tau[r]))).astype(np.int64)
        o = np.lexsort((cols, -img))
        o = o[elig[r][o]][:k]
        out[r, :len(o)] = o
    return out


def chi2_quantile(df, p=0.999):
    """The p quantile of chi^2 at df degrees of freedom (bisection on the regularised incomplete gamma function):
    58.30 at df = 29, the bound of tests/test_slate_sample_cpu.py for its 30 cells."""
    import torch
    lo, hi = 0.0, 10.0 * df + 100.0
    a = torch.tensor(df / 2.0, dtype=torch.float64)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if float(torch.special.gammainc(a, torch.tensor(mid / 2.0, dtype=torch.float64))) < p:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def law_chi2(ids, lp, scores, tau, min_expected=5.0):
    """The law statistic of rows that share one score vector: the chi^2 of the observed ordered k-tuples ids [rows, k]
    against rows * exp(sum logp) as REPORTED with the draw (lp [rows, k]; the mean over the rows that drew the tuple;
    a tuple nobody drew takes the exact value), as slate_sample_oracle.pair_chi2 does for pairs.  With 4096 rows over
    V (V - 1) (V - 2) tuples most cells expect less than one row, where chi^2 is no chi^2: the cells whose EXACT
    expectation is below min_expected are pooled into one (the usual rule of five; the pooling does not look at the
    draws).  -> (chi2, cells, the 0.999 quantile at cells - 1 degrees of freedom: the slate test's bound computed the
    same way for this cell count)."""
    import itertools
    ids = np.asarray(ids)
    rows, k = ids.shape
    V = len(scores)
    L = np.asarray(scores, dtype=np.float32)[None, :]
    all_elig = np.ones((1, V), dtype=bool)
    code = np.zeros(rows, dtype=np.int64)
    for t in range(k):
        code = code * V + ids[:, t]
    total = np.asarray(lp, dtype=np.float64).sum(1)
    chi2, cells, pooled_o, pooled_e, mass = 0.0, 0, 0.0, 0.0, 0.0
    for tup in itertools.permutations(range(V), k):
        exact = float(np.exp(logp(L, all_elig, np.array([tup]), [tau]).sum()))
        mass += exact
        c = 0
        for t in tup:
            c = c * V + t
        hit = code == c
        n = int(hit.sum())
        e = rows * (float(np.exp(total[hit].mean())) if n else exact)
        if rows * exact < min_expected:
            pooled_o += n
            pooled_e += e
            continue
        chi2 += (n - e) ** 2 / e
        cells += 1
    assert abs(mass - 1) < 1e-9
    if pooled_e > 0:
        chi2 += (pooled_o - pooled_e) ** 2 / pooled_e
        cells += 1
    return float(chi2), cells, chi2_quantile(cells - 1)
