"""Which kernel pair of a-recsys_amd/csrc/gru.hip a shape reaches -- the GRU's lstm_paths.py.

arx_gru_fwd and arx_gru_bwd choose among three kernel pairs (four instances) by (din, h) ALONE: there is no four-row
form, so neither B nor the CU count enters, and forward and backward choose by the SAME rule (gru.hip: gru_path).  A
GPU test names the path it is about and asserts it through the functions below, so that a dispatch rule changed later
makes the test fail instead of quietly moving its case to another kernel.  Nothing here is imported by the package.

    'wreg'    k_gru_fwd_wreg<64> / k_gru_bwd_wreg<64>   din == h == 64, weights register-resident
    'mfma1'   k_gru_fwd<1>       / k_gru_bwd<1>         h = 64,  din % 4 == 0, weights streamed
    'mfma2'   k_gru_fwd<2>       / k_gru_bwd<2>         h = 128, din % 4 == 0: two 16-unit tiles per wave
    'generic' k_gru_fwd_generic  / k_gru_bwd_generic    one workgroup per batch row"""

ROWS = 16                       # gru.hip kGruRows: batch rows per workgroup of the wreg and mfma kernels (the MFMA M)
LDS_DEFAULT = 64 * 1024         # dynamic LDS a launch gets without opting in (gru.hip gru_raise_lds)
LDS_LIMIT = 160 * 1024          # gru.hip kGruLdsLimit


def path(din, h):
    """gru.hip gru_path: wreg at din == h == 64, else the streaming MFMA kernels when h in {64, 128} AND
    din % 4 == 0, else generic."""
    if h == 64 and din == 64:
        return 'wreg'
    if h in (64, 128) and din % 4 == 0:
        return 'mfma1' if h == 64 else 'mfma2'
    return 'generic'


fwd_path = bwd_path = path


def fwd_lds_bytes(din, h, p=None):
    """Dynamic LDS of the forward launch (arx_gru_fwd): streaming MFMA -- x and h double-buffered plus r * h_prev,
    16 rows, stride + 2; generic -- the input row and h_prev, 2h gates, h of r * h_prev; wreg: static."""
    p = p or path(din, h)
    if p in ('mfma1', 'mfma2'):
        return 4 * ROWS * (2 * (din + 2) + 3 * (h + 2))
    if p == 'generic':
        return 4 * (din + 4 * h)
    return 0


def bwd_lds_bytes(h, p):
    """Dynamic LDS of the backward launch (arx_gru_bwd): streaming MFMA -- 16 rows of dzc (stride h + 2) and of
    [dzr | dzu] (stride 2h + 2); generic -- h of dzc, 2h of dzg, h of dh, h of the direct part."""
    if p in ('mfma1', 'mfma2'):
        return 4 * ROWS * (3 * h + 4)
    if p == 'generic':
        return 4 * 5 * h
    return 0


# ---------------------------------------------------------------- the shape table of tests/test_gru_kernels_gpu.py
# name -> ([(din, h)], B values, L values)
def table():
    return {
        'wreg': ([(64, 64)], [1, 16, 17, 48], [1, 2, 3]),
        'mfma': ([(4, 64), (68, 64), (64, 128), (132, 128)], [15, 33], [1, 3]),
        'generic': ([(3, 5), (64, 96), (6, 64)], [1, 3], [1, 4]),
    }


def on_path(name, din, h):
    """The caller's `assert on_path(...)`: shape (din, h) runs the kernels that table row `name` is about."""
    p = path(din, h)
    if name == 'mfma':
        return p == ('mfma1' if h == 64 else 'mfma2') and h in (64, 128)
    return p == name
