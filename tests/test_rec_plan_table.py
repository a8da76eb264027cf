"""sbr_rec_plan (csrc/sbr_rec.hip) against the table its predecessors produced.  CPU only: the plan is host code.

tools/rec_plan_table.hip prints the plan over a fixed grid of layer shapes; tests/golden/rec_plan_table.txt holds what the commit
named in its first line answered for the same grid, with its per-family predicates applied in the order its launchers and sbr_query
applied them.  The first tests check that the golden is worth comparing against; the last one builds the program and compares."""
import os
import shutil
import subprocess
from collections import defaultdict

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sequence-based-recommendations_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "rec_plan_table.txt")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = {"triage", "c16", "cl8", "x6p", "x6q", "x6s", "x6", "mfma"}
FAMILY = {"triage": 0, "c16": 1, "cl8": 1, "x6p": 2, "x6q": 3, "x6s": 4, "x6": 4, "mfma": 4}
# outputs that merely scale with the batch or the tile height say nothing about a clause: a pair of rows counts as different
# when one of the others differs
DECIDED = ("fwd", "bwd", "family", "products_fwd", "products_bwd", "bwd_chunkable", "fuse_gather", "tail_ok", "needs_fill", "bwd_dbuf")


@pytest.fixture(scope="module")
def table():
    lines = open(GOLDEN).read().splitlines()
    assert lines[0].startswith("# made by the predicates of commit ")
    def fields(side, names=None):      # a name group "a,b,c" heads a group of one-digit values "010"
        out = []
        for k, w in enumerate(side.split()):
            out += w.split(",") if names is None else (list(w) if "," in names[k] else [w])
        return out
    heads = [s.split() for s in lines[1][2:].split(" | ")]
    ins, outs = (fields(s) for s in lines[1][2:].split(" | "))
    rows = []
    for ln in lines[2:]:
        a, b = (fields(s, h) for s, h in zip(ln.split(" | "), heads))
        assert len(a) == len(ins) and len(b) == len(outs), ln
        rows.append((dict(zip(ins, a)), dict(zip(outs, b))))
    return ins, outs, rows


def test_golden_is_a_few_thousand_distinct_rows(table):
    ins, _, rows = table
    assert 2000 <= len(rows) <= 5000
    assert len({tuple(i[c] for c in ins) for i, _ in rows}) == len(rows)
    assert os.path.getsize(GOLDEN) < 300 * 1024


def test_every_kernel_is_planned_in_both_directions(table):
    _, _, rows = table
    assert {o["fwd"] for _, o in rows} == KERNELS
    assert {o["bwd"] for _, o in rows} == KERNELS


def test_forward_and_backward_can_leave_the_same_family(table):
    _, _, rows = table
    assert any(FAMILY[o["fwd"]] != FAMILY[o["bwd"]] for _, o in rows)           # x6s forward, x6q backward (the fused gather's bound)
    # LSTM, 128 units, 16-row tiles, no pipelined kernels: the forward's LDS fits, the backward's does not
    hit = [o for i, o in rows if (i["cell"], i["Hp"], i["rpt"], i["x6_pipe"]) == ("0", "128", "16", "0") and i["simple"] == "0" and i["f32_mfma"] == "0"]
    assert hit and all((o["fwd"], o["bwd"]) == ("x6", "mfma") for o in hit)
    assert all(o["products_bwd"] == "6" for o in hit)                              # ... and the query still counts bf16x6 products


def test_flags_are_present_both_ways(table):
    _, _, rows = table
    for c in ("simple", "f32_mfma", "prof", "fused", "relu", "x6_pipe", "x6_f16", "x6_f16_bwd", "cl16", "cluster", "contiguous", "xh", "pring", "dh_ext"):
        assert {i[c] for i, _ in rows} == {"0", "1"}, c


def test_the_listed_clause_inputs_are_covered(table):
    _, _, rows = table
    col = lambda c: {i[c] for i, _ in rows}
    assert col("rpt") == {"1", "2", "4", "8", "16"}
    assert col("Hp") == {"16", "32", "48", "64", "128", "256", "304", "512", "1024", "1040"}
    assert col("clip") == {"0", "100", "1000"}
    assert {"4095", "4096", "4097"} <= col("T")
    assert any(int(b) % 8 == 0 and int(b) % 16 for b in col("Bp")) and any(int(b) % 8 for b in col("Bp"))
    assert any(int(b) > 1 << 20 for b in col("Bp")) and any(int(n) > 1 << 20 for n in col("n_in"))      # the 2^32-byte bounds
    assert col("gate_offset") == {"0", "1", "2"}


def test_every_value_of_every_input_decides_something(table):
    """For every input column and every value it takes: two rows that differ in that column ONLY, one of them with that value,
    whose plans differ.  (One row per clause input moved off the base shape's default is how the grid is built.)"""
    ins, _, rows = table
    for k, c in enumerate(ins):
        groups = defaultdict(list)
        for i, o in rows:
            groups[tuple(i[x] for x in ins if x != c)].append((i[c], tuple(o[d] for d in DECIDED)))
        decisive = set()
        for g in groups.values():
            for v, o in g:
                if any(v2 != v and o2 != o for v2, o2 in g):
                    decisive.add(v)
        assert decisive == {i[c] for i, _ in rows}, (c, sorted({i[c] for i, _ in rows} - decisive))


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_plan_equals_the_golden_table(tmp_path):
    if not os.path.exists(os.path.join(os.path.dirname(CSRC), "libsbr_rnn.so")):
        import __graft_entry__
        __graft_entry__.build()
    exe = str(tmp_path / "rec_plan_table")
    env = dict(os.environ)
    env.setdefault("HIPCC", HIPCC if os.path.exists(HIPCC) else "hipcc")
    subprocess.check_call(["make", "-C", CSRC, "plan_table", "PLAN_TABLE=" + exe], env=env, stdout=subprocess.DEVNULL)
    got = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    want = open(GOLDEN).read().splitlines()[1:]
    assert len(got) == len(want)
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, wrong[:5]
