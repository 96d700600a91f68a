"""Frames that name their own packet, in every layout the loaders read.

How a packet's fields get from memory into a lane's registers (csrc/
cop_device.h: load_step / gather_step, load_off_imix / load_step_imix;
csrc/cop_tile.h: the 16- and 12-byte record loads and the per-lane slot
loads of tile_body, the windowed pipelines of tile_steps_v) is otherwise run
on generator traffic only, whose records are one of a dozen values. This
module builds the inputs that test_frame_layouts.py (the module against the
oracle, on the host) and test_gpu_frame_layouts.py (the kernels against the
prescription) share:

  identity      tables and frames such that the record of the packet with
                global index g is a function of g, injective over any window
                of 16,384 indices: the route stage answers g % R + 1, the
                vport and the firewall verdict follow fixed patterns of g
                (R = 4096 keeps the route table in LDS; the vport then tells
                the window's four blocks apart)
  who           a record turned back into the packet that carries it and the
                wave, lane and step that load it
  filler        every byte a loader moves but must ignore (frame bytes
                outside 12..15 and 26..33, the bytes between slots, in front
                of data_off and between IMIX packets) comes from a seeded
                stream; every case runs with two seeds
  slots, imix, hdr16, hdr12
                the device image of a batch in each layout, with the
                make_batch / make_ring keywords
  ethertype_sweep, version_sweep
                every EtherType, every version / IHL byte, with the records
                the contract (include/cop_gpu.h) prescribes
"""
from collections import namedtuple

import numpy as np

import copgpu as cg
import lpm_edges as le
import verdict_patterns as vp

S, F, L = vp.S, vp.F, vp.L
WINDOW = 16384
K = cg.MAX_DEMUX_PORTS                   # vports of the context (n_ports)
NO_PORT_RES = (61, 7)                    # g % 61 == 7: a key whose port is >= n_ports
UNKNOWN_RES = (67, 11)                   # g % 67 == 11: a key with UNKNOWN_PORT
FILL_SEEDS = (0x5EEDF1A1, 0x5EEDF2B2)
GAP_SEED = 0x0A0A0A0A                    # xor: the stream of the bytes outside the frames
FIELD_COLS = np.r_[12:16, 26:34]         # the frame bytes a verdict depends on
IGNORED_COLS = np.setdiff1d(np.arange(64), FIELD_COLS)
# byte classes of a device image (Layout.label)
GAP, HEADROOM, IGNORED, FIELD = 0, 1, 2, 3

IMIX_POLICIES = ("phases", "descending", "shuffled", "min48", "same")

Layout = namedtuple("Layout", "name image label offsets kw shift g")
# image   the bytes at the device buffer, label their classes; pkts = buffer + shift
# offsets u32 per packet or None; kw: stride / data_off for make_batch and make_ring
# g       the global index of the identity frame each packet carries


# ---------------------------------------------------------------------------
# identity

def fw_table() -> cg.LpmTable:
    return cg.LpmTable(vp.fw_rules(), *vp.FW_CFG)


def route_rules(R: int = WINDOW) -> np.ndarray:
    """R /16 prefixes (0x4000 + k) << 16 with next hop k + 1."""
    k = np.arange(R, dtype=np.uint64)
    return le.rows((np.uint64(0x4000) + k) << np.uint64(16), 16, k + np.uint64(1))


def route_table(R: int = WINDOW) -> cg.LpmTable:
    return cg.LpmTable(route_rules(R), 1 << 20, 1 << 16, False)


def routing_table() -> np.ndarray:
    return vp.routing_table(K)


def _u64(g):
    return np.atleast_1d(np.asarray(g, dtype=np.uint64))


def port_of(g, R: int = WINDOW):
    """(vport index, NO_PORT mask, UNKNOWN mask) of global indices g: the
    vport also tells the blocks of R indices inside a window apart."""
    g = _u64(g)
    q = ((g + np.uint64(3) * (g // np.uint64(R))) % np.uint64(K)).astype(np.int64)
    nop = g % np.uint64(NO_PORT_RES[0]) == NO_PORT_RES[1]
    unk = (g % np.uint64(UNKNOWN_RES[0]) == UNKNOWN_RES[1]) & ~nop
    return q, nop, unk


def fw_of(g):
    """(drop mask, accept-rule hit mask) of g: drops at residues of 7 and 5,
    hits of an accepting rule at multiples of 3, misses elsewhere."""
    g = _u64(g)
    drop = (g % np.uint64(7) == 3) | (g % np.uint64(5) == 1)
    hit = ~drop & (g % np.uint64(3) == 0)
    return drop, hit


def addresses(g, R: int = WINDOW):
    """(src, dst) u32 of the identity frames g."""
    g = _u64(g)
    drop, hit = fw_of(g)
    rule = np.full(len(g), -1, dtype=np.int64)
    rule[drop] = np.array(vp.FW_DROP_RULES)[((g[drop] // np.uint64(7)) % np.uint64(3)).astype(np.int64)]
    rule[hit] = np.array(vp.FW_ACCEPT_RULES)[((g[hit] // np.uint64(3)) % np.uint64(3)).astype(np.int64)]
    r = np.maximum(rule, 0)
    base = np.where(rule >= 0, np.array(vp.FW_IP, dtype=np.uint64)[r], np.uint64(vp.SRC_MISS))
    span = np.where(rule >= 0, np.uint64(1) << (np.uint64(32) - np.array(vp.FW_DEPTH, dtype=np.uint64)[r]),
                    np.uint64(1 << 24))
    src = base + (g * np.uint64(2654435761)) % span
    q, nop, unk = port_of(g, R)
    key = np.array(vp.PORT_KEY, dtype=np.uint64)[q]
    key[nop] = vp.NO_PORT_KEY
    key[unk] = vp.UNKNOWN_KEY
    dst = ((np.uint64(0x4000) + g % np.uint64(R)) << np.uint64(16)) | key
    return src.astype(np.uint32), dst.astype(np.uint32)


def records(g, stages: int = S | F | L, R: int = WINDOW, et=None, b14=None) -> np.ndarray:
    """The records the contract prescribes for the identity frames g, whose
    EtherType is et (default 0x0800) and whose byte 14 is b14 (default 0x45)."""
    g = _u64(g)
    n = len(g)
    assert stages & F
    et = np.full(n, 0x0800) if et is None else np.asarray(et)
    b14 = np.full(n, 0x45) if b14 is None else np.asarray(b14)
    q, nop, unk = port_of(g, R)
    rec = np.zeros(n, dtype=cg.RESULT_DT)
    reached = np.ones(n, dtype=bool)
    if stages & S:
        bad_et = et != 0x0800
        rec["port"] = np.where(bad_et | unk, cg.UNKNOWN_PORT, np.where(nop, vp.NO_PORT_VALUE, q))
        rec["verdict"] = np.where(bad_et | unk, cg.DROP_PARSE, np.where(nop, cg.DROP_NO_PORT, cg.FORWARD))
        reached = rec["verdict"] == cg.FORWARD
    drop, hit = fw_of(g)
    v4 = (b14 >> 4) == 4
    rec["verdict"] = np.where(reached, np.where(~v4, cg.DROP_NOT_IPV4, np.where(drop, cg.DROP_FW, cg.FORWARD)),
                              rec["verdict"])
    rec["flags"] = (reached & v4 & (drop | hit)) * cg.FLAG_FW_HIT
    if stages & L:
        rec["flags"] |= (reached * cg.FLAG_ROUTE_HIT).astype(np.uint8)
        rec["route_nh"] = np.where(reached, g % np.uint64(R) + np.uint64(1), 0)
    return rec


def forward_list(rec: np.ndarray) -> np.ndarray:
    return np.nonzero(rec["verdict"] == cg.FORWARD)[0].astype(np.uint32)


def who(rec, lo: int, first: int = 0, ppt: int = 1, R: int = WINDOW, seg_wave: bool = False,
        stages: int = S | F | L, others=()) -> str:
    """The packet whose identity a record carries, among the global indices
    lo .. lo + WINDOW - 1, and where a batch that starts at index `first`
    loads it at 256 * ppt packets per tile: (packet, wave, lane, step).
    seg_wave: the poll-mode step path at 4 packets per lane, where a wave
    walks its own segment (cop_tile.h step_off). Without the parse stage
    no record has a vport: with R < WINDOW the first candidate is named.
    others: (label, first, n) of other batches whose frames a wrong read
    could meet (another slot, the slot's previous lap); a packet of theirs
    is named with its label."""
    nh, port, flags = int(rec["route_nh"]), int(rec["port"]), int(rec["flags"])
    if not (flags & cg.FLAG_ROUTE_HIT) or not 1 <= nh <= R:
        return "no identity frame's record"
    cand = [g for g in range(lo + (nh - 1 - lo) % R, lo + WINDOW, R)]
    if (stages & S) and port < K:
        cand = [g for g in cand if port_of(g, R)[0][0] == port] or cand
    g = cand[0]
    label = ""
    for name, f0, n0 in others:
        if f0 <= g < f0 + n0 and not first <= g < first + n0:
            label, first = f"{name}'s ", f0
    p = g - first
    t = p % (256 * ppt)
    if seg_wave and ppt == 4:
        wave, step = t // 256, (t % 256) // 64
    else:
        step, wave = t // 256, (t % 256) // 64
    return f"{label}packet {p} (identity {g}: tile {p // (256 * ppt)}, wave {wave}, lane {t % 64}, step {step})"


def describe(name, got, want, lo, first=0, ppt=1, R=WINDOW, seg_wave=False, stages=S | F | L, others=()) -> str:
    """The first differing records of a batch, each with the packet it names."""
    bad = np.nonzero(got != want)[0]
    out = [f"{name}: {bad.size} records differ"]
    for j in bad[:4]:
        out.append(f"  packet {j} (tile {j // (256 * ppt)}): gpu {got[j]} is that of "
                   f"{who(got[j], lo, first, ppt, R, seg_wave, stages, others)}; prescribed {want[j]}")
    return "\n".join(out)


# ---------------------------------------------------------------------------
# frames and filler

def frames(g, seed: int, R: int = WINDOW, et=None, b14=None, b15=None) -> np.ndarray:
    """len(g) x 64 bytes: the identity frames g, every byte outside 12..15
    and 26..33 from the stream of `seed`."""
    g = _u64(g)
    src, dst = addresses(g, R)
    f = le.probe_frames(src, dst).reshape(len(g), 64).copy()
    fill = np.random.default_rng(seed).integers(0, 256, (len(g), 64), dtype=np.uint8)
    f[:, IGNORED_COLS] = fill[:, IGNORED_COLS]
    if et is not None:
        f[:, 12], f[:, 13] = np.asarray(et) >> 8, np.asarray(et) & 0xFF
    if b14 is not None:
        f[:, 14] = b14
    if b15 is not None:
        f[:, 15] = b15
    return f


def _canvas(nbytes: int, seed: int):
    img = np.random.default_rng(seed ^ GAP_SEED).integers(0, 256, nbytes, dtype=np.uint8)
    return img, np.full(nbytes, GAP, dtype=np.uint8)


def _place(img, label, starts, fr, width):
    """The first `width` bytes of every frame at its start."""
    at = np.asarray(starts, dtype=np.int64)[:, None] + np.arange(width)
    img[at] = fr[:, :width]
    cls = np.full(64, IGNORED, dtype=np.uint8)
    cls[FIELD_COLS] = FIELD
    label[at] = cls[:width]


def span_of(g) -> int:
    """The start of the window of identities a batch's records are read in."""
    return int(np.min(g))


def slots(n: int, first: int, seed: int, stride: int = 64, data_off: int = 0, R: int = WINDOW, **fields) -> Layout:
    """n slots `stride` bytes apart behind data_off bytes of headroom."""
    g = first + np.arange(n)
    fr = frames(g, seed, R, **fields)
    width = min(64, stride)
    img, label = _canvas(data_off + n * stride, seed)
    label[:data_off] = HEADROOM
    _place(img, label, data_off + np.arange(n, dtype=np.int64) * stride, fr, width)
    return Layout(f"slots({stride},{data_off})", img, label, None, dict(stride=stride, data_off=data_off), 0, g)


def imix_offsets(n: int, policy: str) -> np.ndarray:
    i = np.arange(n, dtype=np.int64)
    if policy == "phases":          # pitches 64, 80, 96, 112 mixed: all four 16-byte phases mod 64
        pitch = 64 + 16 * ((i * 5 + i // 3) % 4)
        return np.concatenate([[0], np.cumsum(pitch)[:-1]])
    if policy == "descending":
        return (n - 1 - i) * 80
    if policy == "shuffled":
        return np.random.default_rng(0x5EEDF303).permutation(n) * 80
    if policy == "min48":
        return i * 48
    assert policy == "same", policy
    return np.full(n, 0x1230)


def imix(n: int, first: int, seed: int, policy: str = "phases", data_off: int = 0, R: int = WINDOW,
         **fields) -> Layout:
    """An IMIX slab with its offsets under a named policy. Under "same" every
    packet is the one frame at that offset."""
    offs = imix_offsets(n, policy)
    g = first + np.arange(n) if policy != "same" else np.full(n, first + 5)
    fr = frames(g, seed, R, **fields)
    width = 48 if policy == "min48" else 64
    img, label = _canvas(data_off + int(offs.max()) + width, seed)
    label[:data_off] = HEADROOM
    _place(img, label, data_off + offs, fr, width)
    return Layout(f"imix({policy},{data_off})", img, label, offs.astype(np.uint32), dict(data_off=data_off), 0, g)


def _host_ptrs(fr: np.ndarray) -> np.ndarray:
    assert fr.flags.c_contiguous and fr.shape[1] == 64
    return fr.ctypes.data + 64 * np.arange(len(fr), dtype=np.uint64)


def hdr16(n: int, first: int, seed: int, R: int = WINDOW, **fields) -> Layout:
    """One 16-byte record per packet (cop_pack_headers)."""
    g = first + np.arange(n)
    fr = frames(g, seed, R, **fields)
    img = cg.pack_headers(_host_ptrs(fr))
    label = np.tile(np.array([FIELD] * 4 + [IGNORED] * 2 + [FIELD] * 8 + [IGNORED] * 2, dtype=np.uint8), n)
    return Layout("hdr16", img, label, None, dict(stride=cg.HDR16_STRIDE), 0, g)


def hdr12(n: int, first: int, seed: int, shift: int = 0, R: int = WINDOW, **fields) -> Layout:
    """One 12-byte record per packet (cop_pack_headers12), the first `shift`
    bytes past a 16-byte boundary."""
    assert shift in (0, 4, 8, 12)
    g = first + np.arange(n)
    fr = frames(g, seed, R, **fields)
    img, label = _canvas(shift + n * cg.HDR12_STRIDE, seed)
    img[shift:] = cg.pack_headers12(_host_ptrs(fr))
    label[shift:] = FIELD
    return Layout(f"hdr12(+{shift})", img, label, None, dict(stride=cg.HDR12_STRIDE), shift, g)


def as_frames(lay: Layout) -> np.ndarray:
    """The layout's packets as n x 64-byte frames read back from its image
    (48 bytes of a frame, the fields of a record; the rest zero): what a
    loader that follows the contract sees."""
    n = len(lay.g)
    out = np.zeros((n, 64), dtype=np.uint8)
    stride, base = lay.kw.get("stride", 64), lay.shift + lay.kw.get("data_off", 0)
    if lay.offsets is None and stride == cg.HDR16_STRIDE:
        r = lay.image[base:base + 16 * n].reshape(n, 16)
        out[:, 12:16], out[:, 24:36] = r[:, :4], r[:, 4:]
    elif lay.offsets is None and stride == cg.HDR12_STRIDE:
        r = lay.image[base:base + 12 * n].reshape(n, 12)
        out[:, 12:16], out[:, 26:34] = r[:, :4], r[:, 4:]
    else:
        st = lay.offsets.astype(np.int64) if lay.offsets is not None else np.arange(n, dtype=np.int64) * stride
        out[:, :48] = lay.image[base + st[:, None] + np.arange(48)]
    return out


def builders(n: int, first: int, seed: int, R: int = WINDOW) -> list:
    """One layout of every kind the GPU tests run."""
    out = [slots(n, first, seed, st, do, R) for st, do in ((64, 0), (48, 16), (80, 48), (112, 0), (2176, 128))]
    out += [imix(n, first, seed, p, do, R) for p in IMIX_POLICIES for do in (0, 16)]
    out.append(hdr16(n, first, seed, R))
    out += [hdr12(n, first, seed, sh, R) for sh in (0, 4, 8, 12)]
    return out


# ---------------------------------------------------------------------------
# header-field sweeps

def ethertype_sweep(seed: int = FILL_SEEDS[0]):
    """(frames, EtherTypes): 65,536 identity frames, bytes 12..13 = i."""
    et = np.arange(65536)
    return frames(et, seed, et=et), et


def ethertype_records(stages: int) -> np.ndarray:
    """With the parse stage an EtherType other than 0x0800 is DROP_PARSE at
    port 0xFFFF; without it nothing reads the EtherType."""
    et = np.arange(65536)
    return records(et, stages, et=et)


def version_sweep(seed: int = FILL_SEEDS[0]):
    """(frames, byte 14): EtherType 0x0800, byte 14 over all 256 values with
    byte 15 0x00, then again with byte 15 0xFF."""
    b14 = np.tile(np.arange(256), 2)
    b15 = np.repeat([0x00, 0xFF], 256)
    return frames(np.arange(512), seed, b14=b14, b15=b15), b14


def version_records(stages: int) -> np.ndarray:
    """A packet that reaches the firewall with (byte 14 >> 4) != 4 is
    DROP_NOT_IPV4; the low nibble and byte 15 change nothing."""
    return records(np.arange(512), stages, b14=np.tile(np.arange(256), 2))
