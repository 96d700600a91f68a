"""The whole-image paint on the host (no GPU): cop_lpm_paint_plan hands out
the intervals and the extended /24 blocks of a table's form, and
cop_paint_host, the paint kernel's mirror (a search per entry inside its
chunk's interval range), paints from them exactly the DIR-24-8 image that
cop_lpm_form_fill_dir24 paints with its running cursor: every tbl24 word,
every tbl8 group, zeros in the spare groups.
"""
import os
import subprocess

import numpy as np
import pytest

import copgpu as cg
import lpm_edges as le
import paint_tables as pt
from live_tables import script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22


def check_table(t: cg.LpmTable):
    """Both forms of t: plan sanity, n_ext, and the two paints word for word."""
    for form in pt.FORMS:
        s, e, x = cg.paint_plan(t, form)
        n_ext = pt.form_n_ext(t, form)
        assert len(x) == n_ext
        assert len(s) == len(e) >= 1 and s[0] == 0 and (np.diff(s.astype(np.int64)) > 0).all()
        want = np.unique(s[(s & 0xFF) != 0] >> 8)
        assert np.array_equal(x, want)
        cap = n_ext + 3
        a24, a8 = pt.fill_dir24(t, form, cap)
        b24, b8 = cg.paint_host(s, e, x, cap, fill=0xABABABAB)
        assert np.array_equal(a24, b24), np.nonzero(a24 != b24)[0][:8]
        assert np.array_equal(a8, b8), np.nonzero(a8 != b8)[0][:8]
        assert not b8[n_ext * 256:].any() and len(b8) == cap * 256
    return s, e, x


def run_script(t: cg.LpmTable):
    g0 = t.generation
    for group in script():
        for op in group:
            if op[0] == "add":
                t.add(*op[1:])
            else:
                t.delete(*op[1:])
    assert t.generation > g0


def test_empty_table():
    t = le.table(le.rows([], [], []))
    s, e, x = check_table(t)
    assert len(s) == 1 and e[0] == 0 and len(x) == 0
    t = cg.LpmTable.empty(1024, 24)
    check_table(t)


EDGE_SETS = {
    "bkt_widths": le.bkt_widths,
    "stride_edges": le.stride_edges,
    "lds_limit": lambda: le.lds_limit(4096),
    "lds_limit_past": lambda: le.lds_limit(4097),
    "routes100k": le.routes100k,
}


@pytest.mark.parametrize("name", list(EDGE_SETS) + ["small_" + k for k in ("crafted", "empty", "halves", "ends", "fw1k")])
def test_every_rule_set_of_lpm_edges(name):
    if name.startswith("small_"):
        rules, cfg = le.small_tables()[name[6:]]
        check_table(le.table(rules, cfg))
    else:
        check_table(le.table(EDGE_SETS[name]()))


def test_crafted_set():
    rules = pt.crafted()
    t = le.table(rules)
    assert t.report.n_added == len(rules)
    s, e, x = check_table(t)
    # the crafted cases are what they claim to be
    assert s[1] == 1 and s[-1] == 0xFFFFFFFF and x[-1] == 0xFFFFFF
    assert (pt.PLAIN_BLOCK << 8) in s and pt.PLAIN_BLOCK not in x
    for a in (0x14000701, 0x14000702, 0x140009FE, 0x140009FF, 0x14000BFF, 0x14000C00):
        assert a in s, hex(a)
    assert 0x140020 in x and 0x140021 in x and 0x140014 in x
    assert ((s >= 0x14001400) & (s < 0x14001500)).sum() == 256
    assert 0x80000000 in s
    C = pt.CHUNK
    for c in pt.EDGE_CHUNKS:
        for b in (c * C - 1, c * C, c * C + 1):
            assert b in x, hex(b)
        assert (c * C << 8) in s
    dense = (s >> 8) // C == pt.DENSE_CHUNK
    assert dense.sum() > 256
    t24, _ = pt.fill_dir24(t, le.FORM_NH, len(x))
    assert (t24[pt.PLAIN_BLOCK] & 0x03000000) == 0x01000000        # valid, not extended
    run_script(t)
    check_table(t)


@pytest.mark.parametrize("name", ["fw2000", "routes20k"])
def test_generated_tables_and_after_mutations(name):
    rules = pt.fw2000() if name == "fw2000" else pt.routes20k()
    t = le.table(rules)
    check_table(t)
    run_script(t)
    check_table(t)


def test_launch_guard():
    s, e, x = cg.paint_plan(le.table(pt.crafted()), le.FORM_NH)
    with pytest.raises(cg.CopError) as err:
        cg.paint_host(s, e, x, len(x) - 1)                      # n_ext > cap_groups
    assert err.value.code == EINVAL
    with pytest.raises(cg.CopError):
        cg.paint_host(s[1:], e[1:], x, len(x))                  # starts[0] != 0
    with pytest.raises(cg.CopError):
        cg.paint_host(s[:0], e[:0], x, len(x))                  # niv == 0
    assert cg.PAINT_CHUNK == 4096 and (1 << 24) % cg.PAINT_CHUNK == 0 and cg.PAINT_CHUNK % 1024 == 0


def test_paint_plan_under_sanitizers(tmp_path):
    """tests/c/paint_plan_check.c, a stand-alone program: the same comparison
    on lpm_build.c + lpm_live.c built with -fsanitize=address,undefined, on
    the crafted set before and after the update script."""
    rules = pt.crafted()
    ops = [op for group in script() for op in group]
    stream = tmp_path / "stream.txt"
    with open(stream, "w") as f:
        f.write(f"{le.RT_CFG[0]} {le.RT_CFG[1]} {len(rules)} {len(ops)}\n")
        for r in rules:
            f.write(f"{int(r['ip'])} {int(r['depth'])} {int(r['next_hop'])}\n")
        for op in ops:
            f.write(f"A {op[1]} {op[2]} {op[3]}\n" if op[0] == "add" else f"D {op[1]} {op[2]} 0\n")
    exe = tmp_path / "paint_plan_check"
    csrc = os.path.join(ROOT, "ghost-dataplane_amd", "csrc")
    cc = subprocess.run(["gcc", "-std=c11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", os.path.join(ROOT, "include"), "-I", csrc,
                         os.path.join(ROOT, "tests", "c", "paint_plan_check.c"), os.path.join(csrc, "lpm_build.c"),
                         os.path.join(csrc, "lpm_live.c"), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe), str(stream)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    t = le.table(rules)
    run_script(t)
    assert f"painted 4 images generation {t.generation}" in run.stdout
