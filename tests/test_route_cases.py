"""The inputs of test_gpu_route_lds.py are what they claim to be
(tests/route_cases.py): for every routing table the oracle (get_next_hop,
switch.c:93-136; fw_packet_handler, firewall.c:170-213) run on the frames
gives exactly the records, the forward list and the counters that the numpy
derivation reads off the table; the tables have the leaf counts and edge
blocks they are there for; the batch looks up every key; and the four
layouts hold the same headers. Conditions on the inputs; the kernels are
checked on the GPU."""
import functools

import numpy as np
import pytest

import copgpu as cg
import oracle as orc
import route_cases as rc
import verdict_patterns as vp
from helpers import oracle_tables

S, F, L = rc.S, rc.F, rc.L


@functools.lru_cache(maxsize=None)
def oracle_twin():
    return oracle_tables(vp.fw_rules(), vp.route_rules(), fw_cfg=vp.FW_CFG)


def assert_records(got, want, what):
    for f in ("verdict", "flags", "port", "route_nh"):
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, f"{what}: {f} at {bad[:8]}: oracle {got[f][bad[:8]]}, derived {want[f][bad[:8]]}"


@pytest.mark.parametrize("stages", [S, S | F | L])
@pytest.mark.parametrize("name", list(rc.TABLES))
def test_oracle_agrees_with_the_derivation(name, stages):
    fw, rt = oracle_twin()
    fr, e = rc.frames(), rc.expected(rc.table(name), stages)
    hits = np.zeros(fw.n_rules, np.uint64)
    ro, fo, co = orc.process(fr.pk, rc.N, rt=rc.table(name), n_ports=rc.N_PORTS, stages=stages,
                             fw=fw if stages & F else None, route=rt if stages & L else None,
                             rule_hits=hits if stages & F else None)
    assert_records(ro, e.rec, name)
    assert np.array_equal(fo, vp.dense_list(e.fwd))
    assert co == e.cnt, (co, e.cnt)
    if stages & F:
        assert np.array_equal(hits, rc.rule_hits(rc.table(name)))


def test_tables_have_their_leaf_counts_and_edges():
    for name, leaves in rc.TABLES.items():
        rt = rc.table(name)
        assert rt.dtype == np.uint16 and rt.shape == (65536,)
        assert rc.leaf_count(rt) == leaves, name
        assert set(np.unique(rt)) <= set(rc.VALUES.tolist())
    blocks = {name: rc.table(name).reshape(256, 256) for name in rc.TABLES}
    uni = blocks["uniform"]
    # uniform blocks with bit 15 set, of every kind
    assert {0x8000, 0xFFFE, 0xFFFF} <= set(uni[:, 0].tolist())

    def differing(b, ref):
        return np.nonzero(b != ref)[0].tolist()
    assert differing(blocks["first"][0], uni[0]) == [0]
    assert differing(blocks["last"][255], uni[255]) == [255]
    assert differing(blocks["three"][0], uni[0]) == [1]
    assert differing(blocks["three"][255], uni[255]) == [254]

    def leaves_of(b):
        return np.nonzero((b != b[:, :1]).any(axis=1))[0].tolist()
    assert leaves_of(blocks["three"]) == [0, 128, 255]
    assert leaves_of(blocks["odd_blocks"]) == list(range(1, 256, 2))
    assert leaves_of(blocks["all_but_one"]) == [b for b in range(256) if b != rc.UNIFORM_MIDDLE]
    # the dense tables use every value in their leaves
    for name in ("odd_blocks", "all_but_one", "all"):
        assert set(np.unique(blocks[name][1])) == set(rc.VALUES.tolist())


def test_frames_look_up_every_key_and_every_class():
    fr = rc.frames()
    assert np.array_equal(np.sort(fr.key[:rc.N_KEYS]), np.arange(65536))
    assert fr.eth_ok[:rc.N_KEYS].all() and fr.ver_ok[:rc.N_KEYS].all()
    f = fr.pk.reshape(rc.N, 64)
    assert (f[:rc.N_KEYS, 14] >> 4 == 4).all() and (f[:rc.N_KEYS, 12] == 8).all() and (f[:rc.N_KEYS, 13] == 0).all()
    dst = f[:, 30:34].copy().view(">u4").ravel()
    assert np.array_equal(dst & 0xFFFF, fr.key)
    assert len(np.unique(dst[:rc.N_KEYS] >> 16)) == 3             # the upper 16 bits vary
    tail = slice(rc.N_KEYS, rc.N)
    assert set((fr.key[tail] >> 8).tolist()) == set(rc.TAIL_BLOCKS)
    assert (~fr.eth_ok[tail]).sum() == 256 and (~fr.ver_ok[tail]).sum() == 256
    for name in rc.TABLES:
        e = rc.expected(rc.table(name), S | F | L)
        # the parse verdict wins over the table: every non-IPv4 frame is DROP_PARSE with UNKNOWN_PORT
        assert (e.rec["verdict"][~fr.eth_ok] == cg.DROP_PARSE).all() and (e.rec["port"][~fr.eth_ok] == 0xFFFF).all()
        # a bad version nibble is judged after the table
        v = e.rec["verdict"][~fr.ver_ok]
        assert set(v.tolist()) <= {cg.DROP_NOT_IPV4, cg.DROP_PARSE, cg.DROP_NO_PORT}
        assert (v == cg.DROP_NOT_IPV4).any()
        for verdict in (cg.FORWARD, cg.DROP_FW, cg.DROP_PARSE, cg.DROP_NOT_IPV4, cg.DROP_NO_PORT):
            assert (e.rec["verdict"] == verdict).any(), (name, verdict)
        assert all(e.cnt[k] > 0 for k in cg.COUNTER_NAMES), (name, e.cnt)
        assert rc.rule_hits(rc.table(name)).min() > 0
        c, lists = rc.port_lists(e)
        assert c.min() > 0 and np.array_equal(np.sort(np.concatenate(lists)), vp.dense_list(e.fwd))
        st = rc.port_stats(e)
        assert np.array_equal(st[:, 1], c) and (st[:, 0] > st[:, 1]).all()


def test_layouts_hold_the_same_headers():
    fw, rt = oracle_twin()
    fr = rc.frames()
    e = rc.expected(rc.table("all"), S | F | L)
    slab, offs = rc.imix()
    assert (offs % 16 == 0).all() and len(np.unique(np.diff(offs.astype(np.int64)))) > 4
    ro, fo, co = orc.process(slab, rc.N, offsets=offs, rt=rc.table("all"), n_ports=rc.N_PORTS, stages=S | F | L,
                             fw=fw, route=rt)
    assert_records(ro, e.rec, "imix")
    assert np.array_equal(fo, vp.dense_list(e.fwd)) and co == e.cnt
    ptrs = fr.pk.ctypes.data + np.arange(rc.N, dtype=np.uint64) * np.uint64(64)
    assert np.array_equal(rc.hdr16(), cg.pack_headers(ptrs))
    assert np.array_equal(rc.hdr12(), cg.pack_headers12(ptrs))
    for name in rc.LAYOUTS:
        data, stride, o = rc.layout(name)
        assert (o is None) == (name != "imix") and stride == {"slots": 64, "imix": 0, "hdr16": 16, "hdr12": 12}[name]
        assert data.nbytes >= rc.N * max(stride, 1)
