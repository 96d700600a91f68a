"""Shared by test_paint_plan.py (host) and test_gpu_table_replace.py (device):
the tables the whole-image paint is checked on, and the reference image.

crafted() puts the paint on its edges: both ends of the address space, starts
at entry 0, 1 and 255 of a /24, a full group, a /1, neighbouring extended
blocks, boundaries either side of a workgroup's chunk of blocks, and a chunk
with more intervals than a workgroup has lanes.
"""
import ctypes

import numpy as np

import copgpu as cg
import lpm_edges as le

FORMS = (le.FORM_NH, le.FORM_RULE)
CHUNK = cg.PAINT_CHUNK
EDGE_CHUNKS = (0x0A1, 0x400)       # boundaries in blocks c*CHUNK - 1, c*CHUNK, c*CHUNK + 1
DENSE_CHUNK = 0x300                # a chunk with more than 256 intervals
PLAIN_BLOCK = 0x140005             # 20.0.5.0/24: a start at a multiple of 256, not extended


def crafted() -> np.ndarray:
    ip, depth, nh = [], [], []

    def add(a, d, h):
        ip.append(a)
        depth.append(d)
        nh.append(h)

    add(0x00000000, 32, 0x100001)                      # the two ends
    add(0xFFFFFFFF, 32, 0x100002)                      # ... and block 0xFFFFFF extended
    add(PLAIN_BLOCK << 8, 24, 0x100003)
    add(0x14000701, 32, 0x100004)                      # starts at x*256 + 1 and + 2
    add(0x140009FE, 32, 0x100005)                      # ... at + 254 and + 255
    add(0x14000BFF, 32, 0x100006)                      # ... at + 255 and the next block's entry 0
    add(0x14001400, 24, 0x100007)                      # a /24 holding 256 /32s
    for o in range(256):
        add(0x14001400 + o, 32, 0x110000 + o)
    add(0x80000000, 1, 0x100008)                       # a /1
    for b in (0x140020, 0x140021):                     # two adjacent extended blocks
        add((b << 8) + 0x80, 25, 0x100009 + (b & 1))
    for c in EDGE_CHUNKS:
        add(((c * CHUNK - 1) << 8) + 5, 32, 0x120000 + c)
        add(((c * CHUNK) << 8) + 0, 32, 0x121000 + c)      # the chunk's first address starts an interval
        add(((c * CHUNK + 1) << 8) + 250, 31, 0x122000 + c)
        add((c * CHUNK + 7) << 8, 24, 0x123000 + c)
    add(EDGE_CHUNKS[1] * CHUNK << 8, 12, 0x100010)     # a prefix that is exactly one chunk
    base = DENSE_CHUNK * CHUNK << 8                    # 300 /32s and 150 /24s in one chunk
    for i in range(300):
        add(base + i * 0xD00 + 3 + (i % 200), 32, 0x130000 + i)
    for i in range(150):
        add(base + 0x80000 + (i << 9), 24, 0x140000 + i)
    return cg.prefixes(ip, depth, nh)


def fill_dir24(t: cg.LpmTable, form: int, cap_groups: int):
    """cop_lpm_form_fill_dir24 on a zero-initialised tbl8 of cap_groups groups."""
    L = cg.lib()
    L.cop_lpm_form_fill_dir24.restype = None
    L.cop_lpm_form_fill_dir24.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    t24 = np.zeros(1 << 24, dtype=np.uint32)
    t8 = np.zeros(max(cap_groups, 1) * 256, dtype=np.uint32)
    L.cop_lpm_form_fill_dir24(t.handle, form, t24.ctypes.data, t8.ctypes.data)
    return t24, t8[: cap_groups * 256]


def form_n_ext(t: cg.LpmTable, form: int) -> int:
    L = cg.lib()
    L.cop_lpm_form_n_ext.restype = ctypes.c_uint32
    L.cop_lpm_form_n_ext.argtypes = [ctypes.c_void_p, ctypes.c_int]
    return int(L.cop_lpm_form_n_ext(t.handle, form))


def fw2000() -> np.ndarray:
    return cg.gen_rules(0x5EED1002, 2000, cg.GEN_FW, 20)


def routes20k() -> np.ndarray:
    return cg.gen_rules(0x5EED2003, 20000, cg.GEN_ROUTES, 0)
