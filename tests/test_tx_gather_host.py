"""cop_tx_gather_host (csrc/tx_gather.c), the tx gather over host memory and
the device kernels' mirror, against a numpy restatement of the semantics in
include/cop_gpu.h (tx_cases.restate): the three list forms, slot and IMIX
sources, the capacity cases, every output extent between 0xAB guards. No GPU.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import copgpu as cg
import tx_cases as tc
import verdict_patterns as vp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
NS = (0, 1, 255, 256, 257, 768, 1027)


def run_and_check(cases, **kw):
    cases = [tc.host_arrays_aligned(c) for c in cases]
    assert tc.run_host(cases, **kw) == 0
    for c in cases:
        c.check(lambda q, k: c.outs[q][k])


@pytest.mark.parametrize("form", ["dense", "seg", "demux"])
@pytest.mark.parametrize("n", NS)
def test_slot_batches_every_mask(n, form):
    K = 5 if form == "demux" else 1
    layouts = vp.port_layouts(n, 256, K) if (K > 1 and n) else {"port0": np.zeros(n, dtype=np.int64)}
    ports = [layouts[k] for k in ("mod", "wave", "port4") if k in layouts] or [layouts["port0"]]
    shapes = [(64, 0, 64, 0), (128, 0, 80, 128), (2176, 128, 2048, 0), (64, 0, 16, 64), (128, 0, 48, 96),
              (2176, 128, 1040, 1088), (2176, 128, 1024, 0)]
    for j, (name, fwd) in enumerate(tc.masks(n).items()):
        stride, data_off, cb, sb = shapes[j % len(shapes)]
        run_and_check([tc.slot_case(n, form, fwd, stride, data_off, cb, sb, ports=ports[j % len(ports)], K=K)])


@pytest.mark.parametrize("form", ["dense", "seg", "demux"])
@pytest.mark.parametrize("n", NS)
def test_imix_batches_every_mask(n, form):
    K = 5 if form == "demux" else 1
    ports = (np.arange(n) // 64) % K
    for j, (name, fwd) in enumerate(tc.masks(n).items()):
        run_and_check([tc.imix_case(n, form, fwd, data_off=16 * (j % 3), ports=ports, K=K, no_off_len=j % 4 == 3)])


def test_imix_lens_are_clamped():
    n = 600
    fwd = vp.patterns(n, 256)["bern_63_64"]
    run_and_check([tc.imix_case(n, "dense", fwd, lens_cycle=(0, 5000, 64, 17))])


@pytest.mark.parametrize("form", ["dense", "seg"])
@pytest.mark.parametrize("src", ["slot", "slot_gap", "imix"])
def test_capacity(src, form):
    n = 1027
    fwd = vp.patterns(n, 256)["bern_63_64"]

    def case_of(caps):
        if src == "imix":
            return tc.imix_case(n, form, fwd, caps=caps)
        return tc.slot_case(n, form, fwd, 128, 0, 80, 80 if src == "slot" else 128, caps=caps)

    for name, c in tc.cap_cases(case_of):
        run_and_check([c])
        st = c.expect[0]["status"][tc.PAD // 4:tc.PAD // 4 + 4]
        assert st[0] + st[2] == len(c.lists[0]), name


def test_several_batches_in_one_call_and_more_than_256_chunks():
    n = vp.LONG_N
    p = vp.patterns(n, 256)
    a = tc.slot_case(n, "seg", p["alt_tile"], 64, 0, 64)
    b = tc.slot_case(1027, "seg", vp.patterns(1027, 256)["seg_tail_k"], 128, 0, 48, 96)
    z = tc.slot_case(0, "seg", np.zeros(0, dtype=bool))
    run_and_check([a, z, b])
    run_and_check([tc.imix_case(n, "dense", p["all"], lens_cycle=(64,))])


def test_einval_leaves_the_outputs_alone():
    n = 300
    fwd = vp.patterns(n, 256)["alt_wave"]

    def bad(mut, form="dense", src="slot", **kw):
        c = tc.imix_case(n, form, fwd) if src == "imix" else tc.slot_case(n, form, fwd, 128, 0, 64, 64)
        c = tc.host_arrays_aligned(c)
        keep = []

        def hold(a):
            keep.append(a)
            return a.ctypes.data

        b, t = c.descs(lambda name: hold(c.inputs[name]), lambda q, k: hold(c.outs[q][k]))
        mut(b, t, c)
        rc = cg.tx_gather_host([b], [t], kw.get("n_lists", c.n_lists), c.seg, kw.get("max_batch", 0))
        assert rc == EINVAL, mut
        for q, o in enumerate(c.outs):   # untouched: still all guard
            for k, v in o.items():
                assert (v.view(np.uint8) == tc.GUARD).all(), (q, k)

    def setf(obj_name, field, value):
        def mut(b, t, c):
            obj = {"b": b, "t": t, "o": t.out[0]}[obj_name]
            setattr(obj, field, value(getattr(obj, field), b, t, c) if callable(value) else value)
        return mut

    bad(setf("b", "fwd_idx", None))
    bad(setf("b", "fwd_count", None))
    bad(setf("b", "stride", 12))
    bad(setf("b", "stride", 120))
    bad(setf("b", "data_off", 8))
    bad(setf("t", "copy_bytes", 0))
    bad(setf("t", "copy_bytes", 40))
    bad(setf("t", "copy_bytes", 144))                      # > stride - data_off
    bad(setf("t", "slot_bytes", 48))                       # < copy_bytes
    bad(setf("t", "slot_bytes", 72))
    bad(setf("t", "lens", lambda v, b, t, c: b.fwd_idx))   # lens on a slot batch
    bad(setf("t", "lens", None), src="imix")
    bad(setf("t", "copy_bytes", 64), src="imix")
    bad(setf("o", "frames", lambda v, b, t, c: v + 8))
    bad(setf("o", "frames", None))
    bad(setf("o", "status", lambda v, b, t, c: v + 4))
    bad(setf("o", "status", None))
    bad(setf("o", "cap_bytes", 1 << 32))
    bad(setf("o", "frames", lambda v, b, t, c: b.pkts + 64))      # output over the packets
    bad(setf("o", "status", lambda v, b, t, c: b.fwd_idx))        # ... over the list
    bad(setf("o", "off", lambda v, b, t, c: b.fwd_count - 16))    # ... its tail over the count
    bad(setf("o", "len", lambda v, b, t, c: t.lens), src="imix")
    bad(lambda b, t, c: None, max_batch=n - 1)
    bad(lambda b, t, c: None, n_lists=9)
    bad(lambda b, t, c: None, form="seg", n_lists=2)
    # n * COP_TX_MAX_FRAME >= 2^32 (nothing is dereferenced before the check)
    bad(setf("b", "n", 1 << 21))
    assert cg.tx_gather_host([], [], 1, False) == 0


def test_struct_layouts_match_c(tmp_path):
    """TxBurst / TxDesc have the C compiler's size and field offsets."""
    mirrors = {"cop_tx_burst": cg.TxBurst, "cop_tx_desc": cg.TxDesc}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cop_gpu.h"', "int main(void){"]
    for cname, py in mirrors.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    lines.append('printf("max_frame %u\\n", COP_TX_MAX_FRAME);')
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
    assert got[("max_frame",)] == cg.TX_MAX_FRAME
    assert ctypes.sizeof(cg.TxBurst) == 48 and ctypes.sizeof(cg.TxDesc) == 16 + 8 * 48


def test_tx_gather_under_sanitizers(tmp_path):
    """tests/c/tx_gather_check.c, a stand-alone program: tx_gather.c built with
    -fsanitize=address,undefined over exactly sized heap blocks, so a byte read
    or written outside an extent stops it."""
    exe = tmp_path / "tx_gather_check"
    csrc = os.path.join(ROOT, "ghost-dataplane_amd", "csrc")
    cc = subprocess.run(["gcc", "-std=c11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", os.path.join(ROOT, "include"), "-I", csrc,
                         os.path.join(ROOT, "tests", "c", "tx_gather_check.c"), os.path.join(csrc, "tx_gather.c"), os.path.join(csrc, "extents.c"),
                         "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "tx_gather_check ok" in run.stdout
