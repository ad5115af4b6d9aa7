"""The float64 oracle of explain_items (arx_explain.h, arx/explain.py): the score of a (row, item) pair as the exact sum

    score(r, c) = 1/F * sum_f s_f(r, c)
       cat feature f:     s_f = u_r . E_f[m_f(c)] + b_f[m_f(c)]
       mulhot feature f:  s_f = 1/len_f(c) * sum_t ( u_r . E_f[v_{f,c,t}] + b_f[v_{f,c,t}] )

restated from tables and CSR maps.  Pure numpy; shared by the CPU and the GPU tests.  A feature is a dict: kind ('cat' |
'mulhot'), E [rows, d], b [rows] or None, and map (cat: int32 [V] or None for the identity) or vals / starts / lens
(mulhot, indexed by logit column)."""
import numpy as np

KEY_NONE = 0x7FFFFFFF
LAYOUTS = {'id': ('cat',), 'mix': ('mulhot',), 'het': ('cat', 'mulhot'), 'ccmm': ('cat', 'cat', 'mulhot', 'mulhot'),
           'f3': ('cat', 'mulhot', 'mulhot')}


def lanes(d):
    """The lanes of one (row, slot) group: the smallest power of two >= d / 4 (arx_explain.h)."""
    L = 1
    while L < d // 4:
        L <<= 1
    return L


def n_cols(feats):
    """The logit columns V the maps of the features cover."""
    ft = feats[0]
    if ft['kind'] == 'mulhot':
        return len(ft['lens'])
    return len(ft['map']) if ft.get('map') is not None else ft['E'].shape[0]


def parts(U, feats, cand):
    """The decomposition in float64.  Returns a dict:
    feat [B, C, F]     1/F * s_f (0 at an empty slot)
    bias [B, C]        1/F * sum_f of the bias part of s_f
    abs_feat [B, C, F] 1/(F * len) * sum over the bag of (sum_i |u_i e_i| + |b|): the scale of feat's rounding bound
    abs_bias [B, C]    1/F * sum_f 1/len * sum over the bag of |b|
    sum_abs_b [B, C]   the plain sum of |b| over every bias term of the item (no coefficients)
    len [B, C, F]      the bag length (1 for a cat feature, 0 at an empty slot)
    tok {(r, j): (val, id, feat, pos, scale)}  one entry per bag position of every mulhot feature, in (feature, position)
                       order: the contribution, the table row, the feature index, the position, and coef * (sum_i
                       |u_i e_i| + |b|), the scale of the contribution's bound.  Empty slots have no key."""
    U = np.asarray(U, dtype=np.float64)
    cand = np.asarray(cand).astype(np.int64)
    B, C = cand.shape
    F = len(feats)
    V = n_cols(feats)
    out = dict(feat=np.zeros((B, C, F)), bias=np.zeros((B, C)), abs_feat=np.zeros((B, C, F)),
               abs_bias=np.zeros((B, C)), sum_abs_b=np.zeros((B, C)), len=np.zeros((B, C, F), dtype=np.int64), tok={}, V=V)
    for r in range(B):
        for j in range(C):
            c = int(cand[r, j])
            if not 0 <= c < V:
                continue
            tv, ti, tf, tp, ts = [], [], [], [], []
            for f, ft in enumerate(feats):
                E = np.asarray(ft['E'], dtype=np.float64)
                b = None if ft.get('b') is None else np.asarray(ft['b'], dtype=np.float64)
                if ft['kind'] == 'cat':
                    rows = np.array([c if ft.get('map') is None else ft['map'][c]], dtype=np.int64)
                else:
                    rows = np.asarray(ft['vals'][ft['starts'][c]:ft['starts'][c] + ft['lens'][c]], dtype=np.int64)
                n = len(rows)
                bb = np.zeros(n) if b is None else b[rows]
                x = E[rows] @ U[r] + bb
                ax = np.abs(E[rows]) @ np.abs(U[r]) + np.abs(bb)
                coef = 1.0 / (F * n)
                out['feat'][r, j, f] = x.sum() * coef
                out['abs_feat'][r, j, f] = ax.sum() * coef
                out['bias'][r, j] += bb.sum() * coef
                out['abs_bias'][r, j] += np.abs(bb).sum() * coef
                out['sum_abs_b'][r, j] += np.abs(bb).sum()
                out['len'][r, j, f] = n
                if ft['kind'] == 'mulhot':
                    tv.append(x * coef); ti.append(rows); tf.append(np.full(n, f)); tp.append(np.arange(n))
                    ts.append(ax * coef)
            cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)
            out['tok'][(r, j)] = (cat(tv, np.float64), cat(ti, np.int64), cat(tf, np.int64), cat(tp, np.int64),
                                  cat(ts, np.float64))
    return out


def top_tokens(p, B, C, T):
    """(val float64 [B, C, T], id int32, feat int32, order {(r, j): the sorted indices into p['tok'][(r, j)]}): the T
    largest contributions by (value desc, feature asc, position asc) -- the entries stand in (feature, position) order,
    so that is a stable sort by value --, (-inf, -1, -1) past the last entry and at an empty slot; a NaN never enters."""
    val = np.full((B, C, T), -np.inf)
    ids = np.full((B, C, T), -1, dtype=np.int32)
    fts = np.full((B, C, T), -1, dtype=np.int32)
    order = {}
    for (r, j), (v, i, f, _, _) in p['tok'].items():
        keep = np.nonzero(~np.isnan(v))[0]
        o = keep[np.argsort(-v[keep], kind='stable')]
        order[(r, j)] = o
        o = o[:T]
        val[r, j, :len(o)], ids[r, j, :len(o)], fts[r, j, :len(o)] = v[o], i[o], f[o]
    return val, ids, fts, order


def bound_tok(d):
    """|got - ref| <= bound_tok(d) * coef * (sum_i |u_i e_i| + |b|): slate_oracle.bound's float32 dot of d terms plus
    the bias (d + 1 roundings), and two more: the rounded coef and the product with it."""
    return 2.0 * (d + 3) * 2.0 ** -24


def bound_feat(d, n):
    """|got - ref| <= bound_feat(d, len) * 1/(F * len) * sum over the bag of (sum_i |u_i e_i| + |b|): the dots and the
    biases as above, len - 1 more roundings of the running sum, the rounded coef and the product; a cat feature is
    len = 1.  n may be an array."""
    return 2.0 * (d + np.asarray(n, dtype=np.float64) + 3) * 2.0 ** -24


def bound_pool_score(d, n, F):
    """The same for the score of score_items, a float32 dot against the POOLED latent: every pool element is a float32
    sum of len rows (len - 1 roundings), a divide, F - 1 adds of the other features and the scale (F + 1 roundings),
    then the dot of d terms and the bias (d + 1): 2 (d + len + F + 2) 2^-24 of the sum of the features' scales, len the
    longest bag of the item.  n may be an array."""
    return 2.0 * (d + np.asarray(n, dtype=np.float64) + F + 2) * 2.0 ** -24


def near_tie(p, order, r, j, T, d):
    """Is the order of the first T tokens of slot (r, j) decided by less than float32 can resolve?  True iff two
    neighbouring contributions among the sorted places 0 .. T (the T kept and the first one left out) lie closer than
    the sum of their two bounds -- unless both are the same table row of the same feature: swapping those changes
    nothing that is compared."""
    v, i, f, _, s = p['tok'][(r, j)]
    o = order[(r, j)][:T + 1]
    for a, b in zip(o[:-1], o[1:]):
        if i[a] == i[b] and f[a] == f[b]:
            continue
        if v[a] - v[b] <= bound_tok(d) * (s[a] + s[b]):
            return True
    return False


# ---------------------------------------------------------------- generators
def bags(rng, V, n_tok, lens):
    """CSR bags of the given lengths [V] over n_tok rows: (vals, starts, lens) int32; tokens may repeat inside a bag."""
    lens = np.asarray(lens, dtype=np.int32)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    vals = rng.integers(0, n_tok, size=int(lens.sum())).astype(np.int32)
    return vals, starts, lens


def forced_lengths(rng, V, forced, lo, hi, choices=None):
    """[V] bag lengths: `forced` at random distinct columns, the rest drawn from `choices` or from [lo, hi]."""
    lens = rng.choice(choices, size=V) if choices is not None else rng.integers(lo, hi + 1, size=V)
    where = rng.choice(V, size=len(forced), replace=False)
    lens[where] = forced
    return lens.astype(np.int32), where


def layout(rng, name, V, n_tok, d, lens_of, dyadic=False, scale=0.5, with_bias=True):
    """The features of LAYOUTS[name] over V logit columns.  The first cat feature is the id row (identity map, V rows),
    a further one maps into 13 rows; every mulhot feature has its own table of n_tok rows and its own bags, of the
    lengths lens_of() returns ([V]).  dyadic: entries k / 2, biases k / 4 (every contribution of a bag whose length is
    a power of two is exact in float32, when F is one too); else scale * N(0, 1)."""
    def table(rows):
        if dyadic:
            return ((rng.integers(-2, 3, size=(rows, d)) / 2.0).astype(np.float32),
                    (rng.integers(-4, 5, size=rows) / 4.0).astype(np.float32) if with_bias else None)
        return ((scale * rng.standard_normal((rows, d))).astype(np.float32),
                (scale * rng.standard_normal(rows)).astype(np.float32) if with_bias else None)
    feats, n_cat = [], 0
    for kind in LAYOUTS[name]:
        if kind == 'cat':
            rows = V if n_cat == 0 else 13
            E, b = table(rows)
            feats.append(dict(kind='cat', E=E, b=b, map=None if n_cat == 0 else
                              rng.integers(0, rows, size=V).astype(np.int32)))
            n_cat += 1
        else:
            E, b = table(n_tok)
            vals, starts, lens = bags(rng, V, n_tok, lens_of())
            feats.append(dict(kind='mulhot', E=E, b=b, vals=vals, starts=starts, lens=lens))
    return feats


def users(rng, B, d, dyadic=False):
    if dyadic:
        return (rng.integers(-2, 3, size=(B, d)) / 2.0).astype(np.float32)
    return rng.standard_normal((B, d)).astype(np.float32)


def slate(rng, B, C, V, must=()):
    """int32 [B, C]: live columns, the `must` columns spread over the first rows, some -1 / V / V + 5 / ARX_KEY_NONE;
    with more than one row the last is all -1."""
    cand = rng.integers(0, V, size=(B, C)).astype(np.int32)
    flat = cand.reshape(-1)
    n_live = (B - 1 if B > 1 else B) * C
    must = np.asarray(must, dtype=np.int32)[:n_live]
    if len(must):
        flat[rng.choice(n_live, size=len(must), replace=False)] = must
    if C >= 4:
        dead = rng.random((B, C)) < 0.1
        dead.reshape(-1)[:n_live][np.isin(flat[:n_live], must)] = False
        cand[dead] = rng.choice([-1, V, V + 5, KEY_NONE], size=int(dead.sum()))
    if B > 1:
        cand[B - 1] = -1
    return cand


def pooled(feats, with_bias=True):
    """(P float64 [V, d], b float64 [V]): the item latent pool the features mean-combine to, for slate_oracle.scores."""
    F = len(feats)
    V = n_cols(feats)
    d = feats[0]['E'].shape[1]
    P, b = np.zeros((V, d)), np.zeros(V)
    for ft in feats:
        E = np.asarray(ft['E'], dtype=np.float64)
        bb = np.zeros(E.shape[0]) if ft.get('b') is None or not with_bias else np.asarray(ft['b'], dtype=np.float64)
        for c in range(V):
            if ft['kind'] == 'cat':
                rows = [c if ft.get('map') is None else ft['map'][c]]
            else:
                rows = ft['vals'][ft['starts'][c]:ft['starts'][c] + ft['lens'][c]]
            P[c] += E[rows].mean(0) / F
            b[c] += bb[rows].mean() / F
    return P, b
