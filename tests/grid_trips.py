"""How far ONE trip of a grid-stride loop reaches, per kernel, as a function of the CU count.

The kernels below launch a grid capped at a multiple of the CU count and walk the rest of their rows in a grid-stride
loop.  A test that wants the loop to take a second and a third trip sizes its shape as 2 * trip + remainder from these
functions, with cu = arx.ops.device_info()["cu_count"] read at run time, and asserts the result (past()), so that a cap
raised later makes the test fail instead of silently covering one trip again.  Every formula restates a launch rule of
a-recsys_amd/csrc and names it; nothing here is imported by the package.  Plain helpers, no fixtures."""

WAVE = 64
BLOCK = 256                     # threads per workgroup of every kernel below (k_pair_auc_counts: 1024)
WAVES_PER_BLOCK = BLOCK // WAVE


def _pow2_lanes(q):
    """The smallest power of two >= q, at most one wave."""
    l = 1
    while l < q and l < WAVE:
        l <<= 1
    return l


def lanes_per_row(d):
    """common.h:49 lanes_per_row: a row of d floats is one float4 per lane of a sub-group of pow2ceil(d / 4) lanes."""
    return _pow2_lanes(d // 4)


def sim_group(d, vec):
    """similar.hip:16 sim_group: the lanes that sum one row -- pow2ceil(d / 4) on the float4 route (d % 4 == 0,
    ld % 4 == 0, 16-byte aligned), pow2ceil(d) on the scalar route, at most 64."""
    return _pow2_lanes(d // 4 if vec else d)


# ---------------------------------------------------------------- pair.hip
def pair_rows(cu, d):
    """k_pair_loss / k_pair_loss_slots -- pair.hip:383-387 (arx_pair_loss_fwdbwd) and :416-420 (arx_pair_loss_slots):
    at most 8 * cu blocks of 4 waves, 64 / LPR rows per wave."""
    return 8 * cu * WAVES_PER_BLOCK * (WAVE // lanes_per_row(d))


PAIR_AUC_ROWS = 256             # k_pair_auc -- pair.hip:438: one block of 256 threads, one row per thread and round
PAIR_AUC_COUNTS_ROWS = 4 * 1024 # k_pair_auc_counts -- pair.hip:213,426: one block of 1024 threads, 4 rows per round


def neg_draw_rows(cu):
    """k_neg_draw_uniform / k_neg_draw_weighted -- pair.hip:451-453 and :469-471: at most 8 * cu blocks of 256
    threads, one row per thread."""
    return 8 * cu * BLOCK


# ---------------------------------------------------------------- window.hip
def window_rows(cu, d):
    """k_gather_window / k_window_slots_bwd -- window.hip:165-169 (arx_gather_window_fwd) and :176-181 (window_grid,
    the two slot calls): the rule of pair_rows."""
    return 8 * cu * WAVES_PER_BLOCK * (WAVE // lanes_per_row(d))


def site_window_items(cu):
    """k_site_window -- window.hip:232-235: at most 8 * cu blocks of 256 threads, one contribution per thread."""
    return 8 * cu * BLOCK


# ---------------------------------------------------------------- slate.hip
SLATE_UNROLL = 4                # slate.hip:16 kSlateUnroll
SLATE_MAX_PASSES = 8            # slate.hip:17 kSlateMaxPasses


def slate_plan(cu, B, C, d):
    """arx_slate_scores -- slate.hip:123-131 -> (passes, run, nruns, units): a wave's run of slots is halved while the
    batch leaves fewer than 64 * cu units; unit w is (row w // nruns, slots [(w % nruns) * run, + run))."""
    per_pass = SLATE_UNROLL * (WAVE // lanes_per_row(d))
    want = cu * 64
    passes = SLATE_MAX_PASSES
    while passes > 1 and B * -(-C // (per_pass * passes)) < want:
        passes >>= 1
    run = per_pass * passes
    nruns = -(-C // run)
    return passes, run, nruns, B * nruns


def slate_units(cu):
    """k_slate_scores -- slate.hip:132-134: at most 16 * cu blocks of 4 waves, one unit per wave."""
    return 16 * cu * WAVES_PER_BLOCK


def slate_merge_items(cu):
    """k_slate_merge_shards -- slate.hip:163-165: at most 16 * cu blocks of 256 threads, one element per thread."""
    return 16 * cu * BLOCK


# ---------------------------------------------------------------- similar.hip
def sim_rows(cu, d, vec):
    """k_rows_inv_norm / k_gather_rows_unit -- similar.hip:106-112 sim_grid: at most 8 * cu blocks of 4 waves,
    64 / L rows per wave, L = sim_group(d, vec)."""
    return 8 * cu * WAVES_PER_BLOCK * (WAVE // sim_group(d, vec))


COS_FINISH_ROWS = 4096          # k_cos_chunk_finish -- similar.hip:162: grid y = min(B, 4096), one row per block
COS_FINISH_COLS = 256 * BLOCK   # similar.hip:160-161: grid x = min(ceil(ncols / 256), 256) blocks of 256 columns


# ---------------------------------------------------------------- shapes
def past(n, trip):
    """n rows take a third trip: the caller's `assert past(n, trip)`."""
    return n > 2 * trip


def slices(n, trip):
    """Three row ranges of at most trip // 2 rows each -- every one a call of one trip: the first rows, a range that
    straddles the end of the first trip, and the last rows with an odd count (a ragged last wave)."""
    h = trip // 2
    assert h >= 2 and past(n, trip)
    a = trip - h // 2
    return [(0, h), (a, a + h), (n - (h - 1), n)]
