"""Host: the identity frames, layout builders and header-field sweeps of
tests/frame_layouts.py against the oracle, before any kernel is judged by
them (test_gpu_frame_layouts.py)."""
import functools

import numpy as np
import pytest

import copgpu as cg
import frame_layouts as fl
import oracle as orc
import verdict_patterns as vp

S, F, L = fl.S, fl.F, fl.L
MASKS = [S | F | L, S | F, F | L]
N = 1500          # packets of a builder's batch: every residue pattern of the identity several times


@functools.lru_cache(maxsize=None)
def oracle_tables(R):
    fw = orc.OracleLpm(*vp.FW_CFG[:2])
    r = vp.fw_rules()
    fw.setup(r["ip"], r["depth"], r["next_hop"])
    rt = orc.OracleLpm(1 << 20, 1 << 16)
    r = fl.route_rules(R)
    rt.setup(r["ip"], r["depth"], r["next_hop"], stop_at_error=False)
    return fw, rt


def oracle_run(fr, stages, R=fl.WINDOW):
    fw, rt = oracle_tables(R)
    return orc.process(np.ascontiguousarray(fr).reshape(-1), len(fr), rt=fl.routing_table(), n_ports=fl.K,
                       stages=stages, fw=fw, route=rt)


def assert_records(name, got, want, lo=0):
    assert np.array_equal(got, want), fl.describe(name, got, want, lo)


@pytest.mark.parametrize("R", [fl.WINDOW, 4096])
def test_identity_is_injective_over_a_window(R):
    """No two of 16,384 consecutive packets share a record, wherever the
    window starts; with the parse stage, among the packets that reach the
    route stage (the others carry the stage's verdict and nothing else).
    With R = 4096 (a route table that stays in LDS) the vport tells the
    window's four blocks apart."""
    for lo in (0, 1, 12345, 3 * fl.WINDOW - 7):
        g = lo + np.arange(fl.WINDOW)
        rec = fl.records(g[:R], F | L, R)       # no vport without the parse stage: a window of R
        assert len(np.unique(rec.view(np.uint64))) == R
        rec = fl.records(g, S | F | L, R)
        reach = (rec["flags"] & cg.FLAG_ROUTE_HIT) != 0
        assert 0.95 < reach.mean() < 0.98
        assert len(np.unique(rec[reach].view(np.uint64))) == reach.sum()
        assert set(np.unique(rec["verdict"])) == {cg.FORWARD, cg.DROP_FW, cg.DROP_PARSE, cg.DROP_NO_PORT}
        assert set(np.unique(rec["port"][reach])) == set(range(fl.K))


def test_verdict_pattern_meets_every_lane_and_tile_phase():
    """The drop residues are coprime to 64 and 256: every lane, and every
    position of a 256-packet step, both drops and forwards."""
    rec = fl.records(np.arange(fl.WINDOW), F | L)
    drop = rec["verdict"] == cg.DROP_FW
    assert 0.2 < drop.mean() < 0.5
    for m in (64, 256):
        per = np.bincount(np.arange(fl.WINDOW) % m, weights=drop, minlength=m)
        assert per.min() > 0 and per.max() < fl.WINDOW // m
    hit = (rec["flags"] & cg.FLAG_FW_HIT) != 0
    assert (hit & ~drop).any() and (~hit & ~drop).any() and hit[drop].all()


def test_who_inverts_the_identity():
    for R, lo, first, ppt in ((fl.WINDOW, 0, 0, 1), (fl.WINDOW, 40000, 40000, 8), (4096, 5000, 5000, 4)):
        g = lo + np.array([0, 1, 63, 64, 255, 256, 2047, 2048, 4095, 4096, 9000, fl.WINDOW - 1])
        stages = F | L if R == fl.WINDOW else S | F | L
        rec = fl.records(g, stages, R)
        for gi, r in zip(g, rec):
            if not r["flags"] & cg.FLAG_ROUTE_HIT:
                continue
            t = (gi - first) % (256 * ppt)
            want = (f"packet {gi - first} (identity {gi}: tile {(gi - first) // (256 * ppt)}, wave {t % 256 // 64}, "
                    f"lane {t % 64}, step {t // 256})")
            assert fl.who(r, lo, first, ppt, R, stages=stages) == want
    r = fl.records([1024 + 256 + 64 + 3], F | L)[0]
    assert "wave 1, lane 3, step 1" in fl.who(r, 0, 0, 4, seg_wave=True)
    assert fl.who(np.zeros(1, cg.RESULT_DT)[0], 0) == "no identity frame's record"
    r = fl.records([3000 + 70], F | L)[0]                       # a stale read: the slot's previous lap
    assert fl.who(r, 0, 6000, 1, others=(("lap 0", 3000, 800),)).startswith("lap 0's packet 70 (identity 3070:")


@pytest.mark.parametrize("stages", MASKS)
@pytest.mark.parametrize("R", [fl.WINDOW, 4096])
def test_oracle_agrees_on_every_builder(stages, R):
    """Every layout's image, read back as the contract says a packet is read
    (as_frames), gives the oracle the prescribed records and forward list,
    with either filler."""
    first = 70000
    for seed in fl.FILL_SEEDS:
        for lay in fl.builders(N, first, seed, R):
            want = fl.records(lay.g, stages, R)
            ro, fo, _ = oracle_run(fl.as_frames(lay), stages, R)
            assert_records(f"{lay.name}/{seed:#x}", ro, want, fl.span_of(lay.g))
            assert np.array_equal(fo, fl.forward_list(want)), lay.name


def test_builder_geometry():
    """Packet starts are 16-byte aligned (12-byte records: 4), IMIX packets
    never overlap, the phases policy meets all four 16-byte phases mod 64
    and the offsets are what their policy says."""
    for p in fl.IMIX_POLICIES:
        o = fl.imix_offsets(N, p)
        assert (o % 16 == 0).all() and len(o) == N
        if p != "same":
            assert np.diff(np.sort(o)).min() >= 48
    o = fl.imix_offsets(N, "phases")
    assert set(o % 64) == {0, 16, 32, 48} and (np.diff(o) > 0).all()
    assert set(o[:64] % 64) == {0, 16, 32, 48}                 # within one wave's step
    assert (np.diff(fl.imix_offsets(N, "descending")) < 0).all()
    assert len(set(fl.imix_offsets(N, "same"))) == 1
    lay = fl.imix(N, 0, fl.FILL_SEEDS[0], "same")
    assert len(set(lay.g)) == 1
    for lay in fl.builders(N, 0, fl.FILL_SEEDS[0]):
        assert lay.image.dtype == np.uint8 and lay.image.shape == lay.label.shape
        assert lay.kw.get("data_off", 0) % 16 == 0


@pytest.mark.parametrize("stages", MASKS)
def test_oracle_agrees_on_the_ethertype_sweep(stages):
    fr, et = fl.ethertype_sweep()
    assert np.array_equal(fr[:, 12].astype(int) << 8 | fr[:, 13], et)
    want = fl.ethertype_records(stages)
    ro, fo, _ = oracle_run(fr, stages)
    for lo in range(0, 65536, fl.WINDOW):
        assert_records(f"ethertype sweep {lo}", ro[lo:lo + fl.WINDOW], want[lo:lo + fl.WINDOW], lo)
    assert np.array_equal(fo, fl.forward_list(want))
    if stages & S:
        # one EtherType passes the parse stage
        assert (want["verdict"] != cg.DROP_PARSE).sum() == 1 and want["verdict"][0x0800] != cg.DROP_PARSE
        assert (want["port"][np.arange(65536) != 0x0800] == 0xFFFF).all()
    else:
        assert np.array_equal(want, fl.records(np.arange(65536), stages))


@pytest.mark.parametrize("stages", MASKS)
def test_oracle_agrees_on_the_version_sweep(stages):
    fr, b14 = fl.version_sweep()
    assert np.array_equal(fr[:, 14], b14) and set(fr[:, 15]) == {0x00, 0xFF}
    want = fl.version_records(stages)
    ro, fo, _ = oracle_run(fr, stages)
    assert_records("version sweep", ro, want)
    assert np.array_equal(fo, fl.forward_list(want))
    v4 = (b14 >> 4) == 4
    reached = ~np.isin(want["verdict"], (cg.DROP_PARSE, cg.DROP_NO_PORT))
    assert ((want["verdict"] == cg.DROP_NOT_IPV4) == (reached & ~v4)).all()
    assert v4.sum() == 32 and (want["verdict"][v4 & reached] != cg.DROP_NOT_IPV4).all()


def test_pack_functions_carry_their_documented_bytes():
    """cop_pack_headers: frame bytes 12..15 then 24..35; cop_pack_headers12:
    12..15 then 26..33; exact, on both sweeps."""
    for fr in (fl.ethertype_sweep()[0], fl.version_sweep()[0], fl.version_sweep(fl.FILL_SEEDS[1])[0]):
        fr = np.ascontiguousarray(fr)
        p16 = cg.pack_headers(fl._host_ptrs(fr)).reshape(-1, 16)
        assert np.array_equal(p16[:, :4], fr[:, 12:16]) and np.array_equal(p16[:, 4:], fr[:, 24:36])
        p12 = cg.pack_headers12(fl._host_ptrs(fr)).reshape(-1, 12)
        assert np.array_equal(p12[:, :4], fr[:, 12:16]) and np.array_equal(p12[:, 4:], fr[:, 26:34])


def test_sweep_layouts_carry_the_sweep():
    """The builders given a sweep's fields hold the sweep's frames."""
    et = np.arange(65536)
    for lay in (fl.slots(65536, 0, fl.FILL_SEEDS[1], 64, 0, et=et), fl.hdr12(65536, 0, fl.FILL_SEEDS[1], 4, et=et),
                fl.imix(65536, 0, fl.FILL_SEEDS[1], "phases", 16, et=et)):
        f = fl.as_frames(lay)
        assert np.array_equal(f[:, 12].astype(int) << 8 | f[:, 13], et), lay.name


def test_filler_seeds_differ_in_every_ignored_byte_class():
    """The two filler seeds give images equal in the field bytes and
    different in (nearly) every byte of each class the loaders must ignore:
    the ignored frame bytes (24..25 and 34..47 among them), the bytes
    between slots, in front of data_off and between IMIX packets."""
    a, b = (fl.frames(np.arange(N), s) for s in fl.FILL_SEEDS)
    assert np.array_equal(a[:, fl.FIELD_COLS], b[:, fl.FIELD_COLS])
    for col in fl.IGNORED_COLS:
        assert (a[:, col] != b[:, col]).mean() > 0.98, col
    seen = set()
    for la, lb in zip(fl.builders(N, 0, fl.FILL_SEEDS[0]), fl.builders(N, 0, fl.FILL_SEEDS[1])):
        assert np.array_equal(la.label, lb.label) and la.name == lb.name
        diff = la.image != lb.image
        assert not diff[la.label == fl.FIELD].any(), la.name
        for c in (fl.GAP, fl.HEADROOM, fl.IGNORED):
            m = la.label == c
            if m.any():
                assert diff[m].mean() > 0.98, (la.name, c)
                seen.add((la.name.split("(")[0], c))
    assert {("slots", fl.GAP), ("slots", fl.HEADROOM), ("slots", fl.IGNORED), ("imix", fl.GAP), ("imix", fl.HEADROOM),
            ("imix", fl.IGNORED), ("hdr16", fl.IGNORED), ("hdr12", fl.GAP)} <= seen
