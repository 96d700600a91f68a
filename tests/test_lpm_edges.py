"""The inputs of test_gpu_lpm_edges.py have the structure they are meant to
have (tests/lpm_edges.py): every crafted rule is accepted, the tables have
the sizes that put them in (or just out of) LDS, the crafted buckets hold
the boundary counts around the bucketed lookup's w > 7 cut, and on the probe
sets the host mirrors of the trie and bucketed forms, the flattened
intervals and the oracle's rte_lpm_lookup restatement all agree. These are
conditions on the inputs; the kernels are checked on the GPU."""
import numpy as np
import pytest

import copgpu as cg
import lpm_edges as le
import oracle as orc


def check_table(rules, cfg=le.RT_CFG, extra=None, cap=None):
    tab = le.table(rules, cfg)
    assert tab.report.n_failed == 0, tab.report.as_dict()
    probes = le.boundary_probes(tab, extra)
    if cap:
        probes = le.subsample(probes, cap)
    assert probes[0] == 0 and probes[-1] == 0xFFFFFFFF and (np.diff(probes.astype(np.int64)) > 0).all()
    nh, hit = le.interval_search(tab, probes)
    for form in (le.FORM_NH, le.FORM_RULE):
        got, ref, info = tab.bkt_probe(probes, form)
        assert np.array_equal(got, ref), ("bkt", form, info)
        got, ref, _, _ = tab.trie_probe(probes, form)
        assert np.array_equal(got, ref), ("trie", form)
    o = orc.OracleLpm(max(cfg[0], len(rules), 1), cfg[1])
    if len(rules):
        o.setup(rules["ip"], rules["depth"], rules["next_hop"], stop_at_error=cfg[2])
    onh, ohit = o.lookup(probes)
    assert np.array_equal(ohit, hit)
    assert np.array_equal(onh[hit == 1], nh[hit == 1])
    return tab, probes


def test_boundary_probes_and_frames():
    r = le.rows([0x0A000000, 0, 0xFFFFFFFF, 0x80000000, 0x0B0C0D0E], [8, 32, 32, 1, 0], [1, 2, 3, 4, 5])
    want = {0x09FFFFFF, 0x0A000000, 0x0A000001, 0x0AFFFFFE, 0x0AFFFFFF, 0x0B000000,     # 10/8
            0xFFFFFFFF, 0, 1, 0xFFFFFFFE,                                                 # the two /32s, wrapping
            0x7FFFFFFF, 0x80000000, 0x80000001}                                           # 128/1; 0/0 adds nothing new
    p = le.boundary_probes(r)
    assert p.dtype == np.uint32 and set(int(x) for x in p) == want
    assert list(p) == sorted(want)
    src = np.array([0x01020304, 0xFFFFFFFF, 0], dtype=np.uint32)
    pk = le.probe_frames(src)
    base = cg.gen_trace(0x5EED0E00, 3, None, None,
                        opts=cg.trace_opts(pct_non_ipv4=0, pct_bad_version=0, pct_unknown_dst=0)).reshape(3, 64)
    f = pk.reshape(3, 64)
    assert (f[:, 12] == 0x08).all() and (f[:, 13] == 0x00).all() and (f[:, 14] >> 4 == 4).all()
    assert list(f[0, 26:30]) == [1, 2, 3, 4] and list(f[0, 30:34]) == [0, 0, 0, 0]
    assert list(f[1, 30:34]) == [255] * 4 and list(f[2, 30:34]) == [1, 2, 3, 4]
    other = np.ones(64, bool)
    other[26:34] = False
    assert np.array_equal(f[:, other], base[:, other])
    slab, offs = cg.gen_imix(0x5EED0E02, 3, None, None)
    le.write_headers(slab, offs, src, src[::-1])
    for i in range(3):
        assert np.array_equal(slab[offs[i] + 26:offs[i] + 34], f[i, 26:34])


def test_bkt_widths_table():
    tab, probes = check_table(le.bkt_widths())
    # 56,249 intervals of the filler + two boundaries for each of the 149 hosts
    # (57,232 if the filler kept 11/8..13/8, which stride_edges needs free)
    assert len(tab.intervals()[0]) == 56547
    info = tab.bkt_probe(probes, le.FORM_NH)[2]
    assert info["ib"] == 17 and info["lifted"] > 0, info
    starts = [0x0A000000 | ((96 + i) << 16) for i in range(len(le.BKT_TARGETS))]
    w = le.bucket_widths(tab, starts)
    assert list(w) == le.BKT_TARGETS
    assert {6, 7, 8, 9, 10, 15, 16, 17} <= set(int(x) for x in w)
    # the firewall's rule-id image of the same prefixes: the same buckets
    fwt = le.table(le.fw_rules(le.bkt_widths()))
    assert fwt.report.n_failed == 0
    assert fwt.bkt_probe(probes, le.FORM_RULE)[2]["ib"] == 17
    assert 150000 < len(probes) < 200000


def test_stride_edges_table():
    tab, probes = check_table(le.stride_edges(), extra=le.STRIDE_EXTRA)
    assert len(tab.intervals()[0]) == 56569
    assert len(probes) == 168918
    # the all-ones path ends in child 63 of every 6-bit level and child 3 of the last
    ip = 0x0CFFFFFF
    assert [(ip >> sh) & m for sh, m in ((14, 63), (8, 63), (2, 63), (0, 3))] == [63, 63, 63, 3]
    nh, hit = le.interval_search(tab, np.array([0x0CFFFFFF, 0x0CFFFFFE, 0x0B000000, 0x0B000001], np.uint32))
    assert list(nh) == [0x030000 + 32, 0x030000 + 31, 0x020000 + 32, 0x020000 + 31] and hit.all()
    # packed tbl8 runs of 13.0.0.0/24 change at entries 1, 2, 31, 32, 33, 34, 63, 64, 65, 255
    t24, t8 = tab.dir24()
    e = t24[0x0D0000]
    assert (e & 0x03000000) == 0x03000000
    g = t8[(e & 0xFFFFFF) * 256:(e & 0xFFFFFF) * 256 + 256]
    assert list(np.nonzero(np.diff(g.astype(np.int64)))[0] + 1) == [1, 2, 31, 32, 33, 34, 63, 64, 65, 255]
    e = t24[0x0D0001]
    g = t8[(e & 0xFFFFFF) * 256:(e & 0xFFFFFF) * 256 + 256]
    assert len(np.unique(g)) == 256


@pytest.mark.parametrize("h,m", [(4095, 8190), (4096, 8192), (4097, 8194)])
def test_lds_limit_tables(h, m):
    rules = le.lds_limit(h)
    assert (rules["ip"] == 0).sum() == 1 and len(np.unique(rules["next_hop"])) == h
    s = np.sort(rules["ip"].astype(np.int64))
    assert (np.diff(s) > 1).all()
    tab, _ = check_table(rules)
    assert len(tab.intervals()[0]) == m
    assert (m <= le.IVT_MAX) == (h <= 4096)
    # as a firewall (rule-id image): no rule's breakpoints merge, the same count
    fwt = le.table(le.fw_rules(rules))
    assert fwt.report.n_failed == 0 and fwt.bkt_probe(np.zeros(1, np.uint32), le.FORM_RULE)[2]["m"] == m


def test_small_tables_and_their_lift_levels():
    lvs = {}
    for name, (rules, cfg) in le.small_tables().items():
        tab, probes = check_table(rules, cfg)
        s, _ = tab.intervals()
        assert len(s) <= le.IVT_MAX, name
        lvs[name] = le.lds_index(s)[3]
        fwt = le.table(le.fw_rules(rules), cfg)
        assert fwt.report.n_failed == 0
    s = le.table(le.stride_edges_crafted()).intervals()[0]
    assert 100 < len(s) < 1000
    for h in (4095, 4096):
        lvs[f"lds_limit({h})"] = le.lds_index(le.table(le.lds_limit(h)).intervals()[0])[3]
    # the LDS lookup's lift loop runs a different number of levels over these
    # tables (never 0: the end sentinel idx[2^ib] = M - 1 >= 3 makes a bucket wide)
    assert len(set(lvs.values())) >= 3, lvs
    assert min(lvs.values()) == 2 and max(lvs.values()) >= 8, lvs


def test_lds_index_restatement_brackets_every_probe():
    """The restated index is the one ivt_search needs: for each probe the
    answer lies in [idx[b], idx[b + 1]] and 2^lv exceeds the widest bucket."""
    for rules in (le.stride_edges_crafted(), le.lds_limit(4096), le.rows([0, 0xFFFFFFFF], [32, 32], [5, 6])):
        tab = le.table(rules)
        s, _ = tab.intervals()
        M, ib, idx, lv = le.lds_index(s)
        probes = le.boundary_probes(tab)
        k = np.searchsorted(s, probes, "right") - 1
        b = probes >> np.uint32(32 - ib)
        assert (idx[b] <= k).all() and (k <= idx[b + 1]).all()
        assert idx[-1] == M - 1 and (1 << lv) > np.diff(idx).max() and idx.max() < 65536


def test_bench_route_table_probes():
    tab, probes = check_table(le.routes100k(), cap=200000)
    assert len(tab.intervals()[0]) > le.IVT_MAX and len(probes) <= 200000
