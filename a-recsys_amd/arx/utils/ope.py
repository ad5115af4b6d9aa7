"""Off-policy evaluation from logged lists (host, numpy, float64): importance weights of whole ordered lists from the
per-entry log-probabilities of list_logprob (the target policy) and of recommend(return_logprob=True) (the logging
policy, written into the log at serving time), and the two usual estimators."""
import numpy as np


def list_weights(logp_target, logp_logged, clip=None):
    """w[r] = pi_target(list r) / pi_logging(list r) = exp(sum_t logp_target[r][t] - sum_t logp_logged[r][t]), float64
    [rows].  A target row sum of -inf (the target policy cannot produce the list) gives weight 0; a logged row sum of
    -inf raises ValueError (the logging policy did produce it).  clip: weights above it are cut to it."""
    t = np.asarray(logp_target, dtype=np.float64)
    g = np.asarray(logp_logged, dtype=np.float64)
    if t.shape != g.shape or t.ndim != 2:
        raise ValueError("list_weights: logp_target and logp_logged [rows, k], got %s and %s" % (t.shape, g.shape))
    if np.isnan(t).any() or np.isnan(g).any():
        raise ValueError("list_weights: NaN log-probabilities")
    ts, gs = t.sum(1), g.sum(1)
    if np.isneginf(gs).any():
        raise ValueError("list_weights: row %d has logged log-probability -inf -- the logging policy did show that "
                         "list" % int(np.nonzero(np.isneginf(gs))[0][0]))
    w = np.zeros(len(ts), dtype=np.float64)
    ok = ~np.isneginf(ts)
    w[ok] = np.exp(ts[ok] - gs[ok])
    return w if clip is None else np.minimum(w, float(clip))


def ips(rewards, w):
    """The inverse-propensity estimate of the target policy's mean reward: mean(w * rewards)."""
    return float(np.mean(np.asarray(w, dtype=np.float64) * np.asarray(rewards, dtype=np.float64)))


def snips(rewards, w):
    """The self-normalised estimate: sum(w * rewards) / sum(w); ValueError when every weight is 0."""
    w = np.asarray(w, dtype=np.float64)
    if not w.sum() > 0:
        raise ValueError("snips: every weight is 0")
    return float(np.sum(w * np.asarray(rewards, dtype=np.float64)) / w.sum())
