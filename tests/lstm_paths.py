"""Which kernel pair of a-recsys_amd/csrc/lstm.hip a shape reaches, as a function of the CU count.

arx_lstm_fwd and arx_lstm_bwd choose among five kernel pairs; forward and backward choose by DIFFERENT rules.  A GPU
test names the path it is about and asserts it through the functions below, with cu = arx.ops.device_info()
["cu_count"] read at run time, so that a dispatch rule changed later makes the test fail instead of quietly moving its
case to another kernel.  Every function restates a rule of lstm.hip and names it; nothing here is imported by the
package.  Plain helpers, no fixtures.

    'r4'      k_lstm_fwd_r4<64>   / k_lstm_bwd_r4<64>     four batch rows per workgroup
    'wreg'    k_lstm_fwd_wreg<64> / k_lstm_bwd_wreg<64>   sixteen rows, W register-resident
    'mfma1'   k_lstm_fwd<1>       / k_lstm_bwd<1>         h = 64, W streamed
    'mfma2'   k_lstm_fwd<2>       / k_lstm_bwd<2>         h = 128, W streamed
    'generic' k_lstm_fwd_generic  / k_lstm_bwd_generic    one workgroup per batch row"""

ROWS = 16                       # lstm.hip:43 kRows: batch rows per workgroup of the wreg and mfma kernels (the MFMA M)
ROWS_R4 = 4                     # lstm.hip:436 kR4: batch rows per workgroup of the r4 kernels
LDS_DEFAULT = 64 * 1024         # dynamic LDS a launch gets without opting in (lstm.hip:718 raise_lds)
LDS_LIMIT = 160 * 1024          # lstm.hip:716 kLdsLimit


def _r4(cu, B, din, h):
    """lstm.hip:738 (forward) and :769 (backward), the same rule: four-row workgroups while sixteen-row ones would
    put fewer than two on a CU."""
    return h == 64 and din == 64 and -(-B // ROWS) < 2 * cu


def fwd_path(cu, B, din, h):
    """arx_lstm_fwd -- lstm.hip:736-756: r4, else wreg at din == h == 64, else the streaming MFMA kernels when
    h in {64, 128} AND din % 4 == 0 (:736), else generic."""
    if _r4(cu, B, din, h):
        return 'r4'
    if h == 64 and din == 64:
        return 'wreg'
    if h % 64 == 0 and h <= 128 and din % 4 == 0:
        return 'mfma1' if h == 64 else 'mfma2'
    return 'generic'


def bwd_path(cu, B, din, h):
    """arx_lstm_bwd -- lstm.hip:768-789: as forward, but the streaming MFMA kernels take ANY din (:768: the backward
    recurrence never touches the x rows of W)."""
    if _r4(cu, B, din, h):
        return 'r4'
    if h == 64 and din == 64:
        return 'wreg'
    if h % 64 == 0 and h <= 128:
        return 'mfma1' if h == 64 else 'mfma2'
    return 'generic'


def wreg_min_B(cu):
    """The first batch size at din == h == 64 that leaves r4: ceil(B / 16) >= 2 * cu  <=>  B >= 32 * cu - 15."""
    return 32 * cu - 15


def fwd_lds_bytes(din, h, path):
    """Dynamic LDS of the forward launch -- lstm.hip:745 (streaming MFMA: x and h double-buffered, 16 rows, stride
    + 2) and :752 (generic: the input row, 4h pre-activations, h cells); the other kernels' LDS is static."""
    if path in ('mfma1', 'mfma2'):
        return 4 * (2 * ROWS * (din + 2) + 2 * ROWS * (h + 2))
    if path == 'generic':
        return 4 * (din + h + 4 * h + h)
    return 0


def bwd_lds_bytes(h, path):
    """Dynamic LDS of the backward launch -- lstm.hip:782 (streaming MFMA: 16 rows of dz, stride 4h + 2) and :770
    (generic: 4h of dz, h of dh, h of dc)."""
    if path in ('mfma1', 'mfma2'):
        return 4 * ROWS * (4 * h + 2)
    if path == 'generic':
        return 4 * 6 * h
    return 0


# ---------------------------------------------------------------- the shape table of tests/test_lstm_kernels_gpu.py
# name -> ((forward path, backward path), [(din, h)], B values as functions of cu, L values)
def table(cu):
    w = wreg_min_B(cu)
    return {
        'r4': (('r4', 'r4'), [(64, 64)], [1, 3, 4, 5, 7, 66, w - 1], [1, 2, 5]),
        'wreg': (('wreg', 'wreg'), [(64, 64)], [w, w + 15, w + 24], [1, 3]),
        'mfma1': (('mfma1', 'mfma1'), [(4, 64), (32, 64), (68, 64), (128, 64)], [1, 15, 16, 17, 33], [1, 2, 5]),
        'mfma2': (('mfma2', 'mfma2'), [(4, 128), (128, 128), (132, 128)], [1, 15, 16, 17, 33], [1, 2, 5]),
        'genfwd': (('generic', 'mfma'), [(1, 64), (18, 64), (63, 128)], [1, 17], [1, 2, 5]),
        'generic': (('generic', 'generic'), [(20, 24), (64, 32), (7, 1), (64, 192), (36, 260)], [1, 5], [1, 2, 5]),
    }


def on_path(cu, name, B, din, h):
    """The caller's `assert on_path(...)`: shape (B, din, h) runs the kernels that table row `name` is about."""
    want_f, want_b = table(cu)[name][0]
    if want_b == 'mfma':
        want_b = 'mfma1' if h == 64 else 'mfma2'
    return fwd_path(cu, B, din, h) == want_f and bwd_path(cu, B, din, h) == want_b
