"""cop_fwd_check_host / cop_fwd_rewrite_host / cop_ipv4_csum_host (csrc/fwd.c),
the host mirror of the L3 forward kernels, against the numpy restatement in
fwd_cases.py. No GPU."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import copgpu as cg
import fwd_cases as fc
import sketch_cases as sc
import tx_cases as tc
import verdict_patterns as vp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
KP = {"dense": 1, "seg": 1, "demux": 5}
FORMS = ("dense", "seg", "demux")
PAD = fc.PAD


def mask_of(n, j):
    names = list(tc.masks(n))
    return tc.masks(n)[names[j % len(names)]]


def run_check(cases):
    bs, ds, _, _, keep = fc.host_descs(cases)
    c = cases[0]
    rc = cg.fwd_check_host(c.table, c.cfg(), bs, ds, c.n_lists, c.seg)
    assert rc == 0
    for x in cases:
        x.expect_check()
        x.check(lambda q, k, x=x: x.outs[0][k])


def run_rewrite(cases, times=1):
    bs, _, ts, rs, keep = fc.host_descs(cases)
    c = cases[0]
    for _ in range(times):
        assert cg.fwd_rewrite_host(c.table, c.cfg(), bs, ts, rs, c.n_lists, c.seg) == 0
    for x in cases:
        x.expect_rewrite(times)
        x.check(lambda q, k, x=x: x.outs[0][k])


# ---- 1. the mirror against the restatement ------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", sc.NS)
def test_check_every_form_layout_flag_and_miss(n, form):
    for j, (layout, flags, miss) in enumerate(itertools.product(fc.LAYOUTS, (0, cg.FWD_VERIFY_CSUM), fc.MISS)):
        c = fc.FwdCase(n, layout, form, mask_of(n, j), KP[form], seed=j, flags=flags, miss=miss, exc=j % 3 != 2)
        run_check([c])
        if n >= 63:
            seen = set(c.prescribed.tolist())
            assert seen == set(range(8)), seen            # every class is prescribed in every case


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", sc.NS)
def test_rewrite_every_form_layout_flag_and_miss(n, form):
    for j, (layout, flags, miss) in enumerate(itertools.product(fc.LAYOUTS, (0, cg.FWD_VERIFY_CSUM), fc.MISS)):
        c = fc.FwdCase(n, layout, form, mask_of(n, j + 1), KP[form], seed=j, flags=flags, miss=miss).with_tx(port=j % 2 == 0)
        run_rewrite([c])
        if n >= 257 and j == 0:
            st = c.expect[0]["rw_status0"][PAD // 4:PAD // 4 + 4]
            assert st[0] > 0 and st[1] > 0 and st[2] > 0, st


@pytest.mark.parametrize("form", FORMS)
def test_many_chunks_several_batches_and_clamps(form):
    n, K = vp.LONG_N, KP[form]
    a = fc.FwdCase(n, "s64", form, vp.patterns(n, 256)["alt_tile"], K, seed=1, flags=cg.FWD_VERIFY_CSUM)
    b = fc.FwdCase(n, "imix", form, vp.patterns(n, 256)["all"], K, seed=2, flags=cg.FWD_VERIFY_CSUM)
    c = fc.FwdCase(600, "s128", form, vp.patterns(600, 256)["all"], K, seed=3, flags=cg.FWD_VERIFY_CSUM)
    c.inputs["counts"][:] = 0xFFFFFFF0                       # counts above what the layout holds
    junk = c.inputs["idx"] == tc.JUNK
    c.inputs["idx"][junk] = 600 + 5 + np.arange(junk.sum())
    c.inputs["idx"][::7] += 600                              # indices >= n
    run_check([a, fc.FwdCase(0, "s64", form, K=K, flags=cg.FWD_VERIFY_CSUM), b, c])
    assert 0 < a.check_status()[0][0] < a.inputs["counts"].sum()


@pytest.mark.parametrize("layout", list(fc.LAYOUTS))
def test_rewrite_capacity_cuts(layout):
    """W below the list's length: frames at or past W, their port words and all guards stay."""
    n = 700
    fwd = vp.patterns(n, 256)["all"]
    for name, c in tc.cap_cases(lambda caps: fc.FwdCase(n, layout, "dense", fwd, seed=5).with_tx(caps).tx):
        case = fc.FwdCase(n, layout, "dense", fwd, seed=5).with_tx(c.caps)
        run_rewrite([case])
    seg = fc.FwdCase(n, layout, "seg", vp.patterns(n, 256)["alt_wave"], seed=6)
    full = fc.FwdCase(n, layout, "seg", vp.patterns(n, 256)["alt_wave"], seed=6).with_tx().tx
    used = int(full.expect[0]["status"][PAD // 4 + 1])
    run_rewrite([seg.with_tx([(used // 2 & ~15, 10_000)])])
    assert 0 < seg.expect[0]["tx_status0"][PAD // 4] < len(seg.true_lists[0])


def test_rewrite_without_records_and_twice():
    c = fc.FwdCase(300, "s64", "dense", seed=7, with_results=False).with_tx()
    run_rewrite([c])
    d = fc.FwdCase(300, "imix", "dense", seed=8).with_tx()
    run_rewrite([d], times=2)                                # TTL 2 frames are TTL class the second time
    st = d.expect[0]["rw_status0"][PAD // 4:PAD // 4 + 4]
    assert st[2] > 0


# ---- 2. checksums -----------------------------------------------------------------------------------------------
def header(rng, ttl):
    h = rng.integers(0, 256, 34, dtype=np.uint8)
    h[12:15] = (0x08, 0x00, 0x45)
    h[22] = ttl
    return h


def rewritten(h, table, flags=0):
    """One 64-byte slot frame through cop_tx-less rewrite: a burst of one frame."""
    fr = tc.aligned(64)
    fr[:34], fr[34:] = h, 0
    idx, cnt = np.zeros(1, np.uint32), np.ones(1, np.uint32)
    st, rst, port = tc.aligned(16).view(np.uint32), tc.aligned(16).view(np.uint32), np.zeros(1, np.uint32)
    st[:] = (1, 64, 0, 0)
    pk = tc.aligned(64)
    b = cg.Batch()
    b.pkts, b.fwd_idx, b.fwd_count, b.n, b.stride = pk.ctypes.data, idx.ctypes.data, cnt.ctypes.data, 1, 64
    t = cg.make_tx(dict(frames=fr.ctypes.data, off=None, len=None, status=st.ctypes.data, cap_bytes=64, cap_frames=1),
                   copy_bytes=64)
    r = cg.make_fwd_rw(rst.ctypes.data, port.ctypes.data)
    assert cg.fwd_rewrite_host(table, cg.fwd_config(flags, 0), [b], [t], [r]) == 0
    return fr, rst.copy()


def test_checksum_every_ttl_and_corner():
    rng = np.random.default_rng(11)
    table = fc.make_table(4)
    for ttl in range(2, 256):
        for corner in (0, 1, 2):
            h = header(rng, ttl)
            pk = h.copy()
            fc.set_valid_header(pk, np.zeros(1, np.int64), np.uint8(ttl), np.array([corner]))
            old = (int(pk[24]) << 8) | int(pk[25])
            assert cg.ipv4_csum_host(pk[14:34]) == old
            fr, st = rewritten(pk, table, cg.FWD_VERIFY_CSUM)
            assert st.tolist() == [1, 0, 0, 0]
            new = (int(fr[24]) << 8) | int(fr[25])
            assert fr[22] == ttl - 1 and new == cg.ipv4_csum_host(fr[14:34]), (ttl, corner, hex(old), hex(new))
            if corner == 1:
                assert new == 0x0000                         # where an RFC 1141-style HC + 0x0100 gives 0xFFFF
                assert int(fc.fold(old + 0x0100)) == 0xFFFF
            if corner == 2:
                assert old == 0x0000
            assert np.array_equal(fr[:12].view(np.uint8), np.concatenate([table["dst_mac"][0], table["src_mac"][0]]))
            assert np.array_equal(fr[12:22], pk[12:22]) and fr[23] == pk[23] and np.array_equal(fr[26:34], pk[26:34])


def test_invalid_checksum_without_verify_gets_eqn_3():
    rng = np.random.default_rng(12)
    table = fc.make_table(4)
    for ttl in (2, 3, 64, 255):
        for _ in range(40):
            h = header(rng, ttl)                              # bytes 24..25 random: invalid but for 1 in 65536
            fr, st = rewritten(h, table, 0)
            assert st.tolist() == [1, 0, 0, 0]
            want = fc.rewrite_rows(h[None, :], table[:1])[0]
            assert np.array_equal(fr[:34], want)
            fr2, st2 = rewritten(h, table, cg.FWD_VERIFY_CSUM)
            if cg.ipv4_csum_host(h[14:34]) != ((int(h[24]) << 8) | int(h[25])):
                assert st2.tolist() == [0, 0, 1, 0] and np.array_equal(fr2[:34], h)


# ---- 3. argument errors ----------------------------------------------------------------------------------------------
def test_einval_leaves_every_array_alone():
    n = 300
    fresh = lambda layout="s128", m=n, form="dense", K=1: fc.FwdCase(m, layout, form, vp.patterns(m, 256)["alt_wave"], K,
                                                                     seed=1).with_tx()

    def refused(cases, mut=None, which="both", max_batch=0, n_lists=None, seg=None, n_entries=None, cfg=None):
        bs, ds, ts, rs, keep = fc.host_descs(cases)
        c = cases[0]
        if mut:
            mut(bs[0], ds[0], ts[0], rs[0], c)
        snap, tab = fc.snapshot(cases), c.table.copy()
        nl, sg = c.n_lists if n_lists is None else n_lists, c.seg if seg is None else seg
        cf = cfg or c.cfg()
        if which in ("both", "check"):
            assert cg.fwd_check_host(c.table, cf, bs, ds, nl, sg, max_batch, n_entries) == EINVAL, mut
        if which in ("both", "rewrite"):
            assert cg.fwd_rewrite_host(c.table, cf, bs, ts, rs, nl, sg, max_batch, n_entries) == EINVAL, mut
        fc.unchanged(cases, snap)
        assert np.array_equal(c.table, tab)

    def setf(which, field, value, q=None):
        def mut(b, d, t, r, c):
            obj = {"b": b, "d": d, "t": t, "r": r}[which]
            if which == "t" and q is not None:
                obj = obj.out[q]
            if which == "r":
                arr = getattr(obj, field)
                arr[0] = value(arr[0], b, d, t, r) if callable(value) else value
                return
            setattr(obj, field, value(getattr(obj, field), b, d, t, r) if callable(value) else value)
        return mut

    refused([fresh(m=4097)], max_batch=4096)                                      # n > max_batch
    refused([fresh()], n_entries=0)
    refused([fresh()], n_entries=(1 << 24) + 1)
    refused([fresh()], cfg=cg.fwd_config(2, 0))                                   # unknown flags
    refused([fresh()], n_lists=0)
    refused([fresh()], n_lists=9)
    refused([fresh()], n_lists=2, seg=True)
    for m in (setf("b", "pkts", None), setf("b", "fwd_idx", None), setf("b", "fwd_count", None),
              setf("b", "pkts", lambda v, *a: v + 8), setf("b", "data_off", 8), setf("b", "stride", 120),
              setf("b", "results", lambda v, *a: v + 4)):
        refused([fresh()], m)
    for stride in (16, 32):                                                       # header records are not taken
        refused([fresh()], setf("b", "stride", stride))
    for m in (setf("d", "out_idx", None), setf("d", "out_count", None), setf("d", "status", None),
              setf("d", "status", lambda v, *a: v + 4), setf("d", "exc_idx", None), setf("d", "exc_count", None),
              setf("d", "lens", lambda v, b, d, t, r: b.fwd_idx),                 # lens on a slot batch
              setf("d", "out_idx", lambda v, b, *a: b.fwd_idx), setf("d", "out_idx", lambda v, b, *a: b.fwd_idx + 4 * (n - 1)),
              setf("d", "out_count", lambda v, b, *a: b.fwd_count), setf("d", "status", lambda v, b, *a: b.pkts + 64),
              setf("d", "exc_count", lambda v, b, *a: b.results + 8), setf("d", "exc_idx", lambda v, b, d, *a: d.out_idx),
              setf("d", "status", lambda v, b, d, *a: d.exc_idx + 16)):
        refused([fresh()], m, "check")
    refused([fresh("imix")], setf("d", "lens", None), "check")                   # IMIX without lens
    tab_case = fresh()
    refused([tab_case], setf("d", "status", tab_case.table.ctypes.data + 16), "check")     # over the table
    two = [fresh(), fresh()]
    bs, ds, ts, rs, keep = fc.host_descs(two)
    ds[1].out_count = ds[0].out_count                                             # two batches' outputs on each other
    assert cg.fwd_check_host(two[0].table, two[0].cfg(), bs, ds) == EINVAL
    rs[1].status[0] = rs[0].status[0]
    assert cg.fwd_rewrite_host(two[0].table, two[0].cfg(), bs, ts, rs) == EINVAL
    for m in (setf("t", "copy_bytes", 32), setf("t", "copy_bytes", 40), setf("t", "slot_bytes", 100),
              setf("t", "frames", None, 0), setf("t", "status", None, 0), setf("t", "frames", lambda v, *a: v + 8, 0),
              setf("t", "cap_bytes", 1 << 32, 0), setf("r", "status", None), setf("r", "status", lambda v, *a: v + 4),
              setf("r", "port", lambda v, *a: v + 2), setf("r", "status", lambda v, b, d, t, r: t.out[0].status),
              setf("r", "port", lambda v, b, d, t, r: t.out[0].frames + 64),
              setf("r", "status", lambda v, b, *a: b.fwd_count), setf("r", "port", lambda v, b, *a: b.results),
              setf("t", "frames", lambda v, b, *a: b.fwd_idx, 0)):
        refused([fresh()], m, "rewrite")
    for m in (setf("t", "off", None, 0), setf("t", "len", None, 0), setf("t", "lens", None)):
        refused([fresh("imix")], m, "rewrite")                                    # an IMIX burst without off / len
    tab_case = fresh()
    refused([tab_case], setf("r", "status", tab_case.table.ctypes.data), "rewrite")
    # nothing to do: 0
    c = fresh()
    assert cg.fwd_check_host(c.table, c.cfg(), [], []) == 0
    assert cg.fwd_rewrite_host(c.table, c.cfg(), [], [], []) == 0


def test_struct_layouts_match_c(tmp_path):
    """The mirrored structs have the C compiler's size and field offsets, the constants its values."""
    mirrors = {"cop_neigh_entry": cg.NeighEntry, "cop_fwd_config": cg.FwdConfig, "cop_fwd_check_desc": cg.FwdCheckDesc,
               "cop_fwd_rw_desc": cg.FwdRwDesc}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cop_gpu.h"', "int main(void){"]
    for cname, py in mirrors.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    consts = ["OK", "PASS", "SHORT", "BAD_HDR", "OPTIONS", "BAD_CSUM", "TTL", "NO_NEIGH", "VERIFY_CSUM", "NO_NH"]
    for k in consts:
        lines.append(f'printf("const {k} %u\\n", COP_FWD_{k});')
    lines.append('printf("const NEIGH_VALID %u\\n", COP_NEIGH_VALID);')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {tuple(l.split()[:-1]): int(l.split()[-1]) for l in out if l.strip()}
    for cname, py in mirrors.items():
        assert got[(cname, "size")] == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert got[(cname, f)] == getattr(py, f).offset, (cname, f)
    for k in consts:
        assert got[("const", k)] == getattr(cg, "FWD_" + k), k
    assert got[("const", "NEIGH_VALID")] == cg.NEIGH_VALID
    assert cg.NEIGH_DT.itemsize == ctypes.sizeof(cg.NeighEntry) == 16


def test_fwd_under_sanitizers(tmp_path):
    """tests/c/fwd_check.c, a stand-alone program: fwd.c (and tx_gather.c, whose
    argument checks and gather it calls) built with -fsanitize=address,undefined
    over exactly sized heap blocks, so a byte read or written outside an extent
    stops it."""
    probe = subprocess.run(["gcc", "-fsanitize=address,undefined", "-x", "c", "-", "-o", str(tmp_path / "probe")],
                           input="int main(void){return 0;}\n", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("gcc's sanitizer runtime is not installed")
    exe = tmp_path / "fwd_check"
    csrc = os.path.join(ROOT, "ghost-dataplane_amd", "csrc")
    cc = subprocess.run(["gcc", "-std=c11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", os.path.join(ROOT, "include"), "-I", csrc,
                         os.path.join(ROOT, "tests", "c", "fwd_check.c"), os.path.join(csrc, "fwd.c"),
                         os.path.join(csrc, "tx_gather.c"), os.path.join(csrc, "extents.c"), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "fwd_check ok" in run.stdout
