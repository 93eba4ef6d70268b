"""The size queries of the packed J/K (host arithmetic: no GPU, no context) answer what tests/golden/jk_packed_sizes.json
recorded, for every n in 0 .. 420, under the default and under every switch setting of jk_cases.SIZE_SETTINGS: the
support class, the fold, the route, the Dtot' table's bytes, and the packed tensor's and the workspace's bytes over the
whole tensor and over three slabs.  The file was written once from the library before csrc/jk_packed.hip's single
resolver replaced the hand-written cascades (tests/golden/make_jk_packed_sizes.py; the commit is in the file), so the
dispatcher is held to its predecessor's answers, quirks included."""

import json

import pytest

import jk_cases as jc
from conftest import GOLDEN


@pytest.fixture(scope="module")
def recorded():
    return json.loads((GOLDEN / "jk_packed_sizes.json").read_text())


def test_the_file_covers_every_size_and_setting(recorded):
    assert recorded["n"] == [0, jc.SIZE_RANGE - 1] and len(recorded["commit"]) == 40
    assert list(recorded["settings"]) == jc.SIZE_SETTINGS and len(jc.SIZE_SETTINGS) == 5
    assert recorded["slabs"] == [[list(s) for s in jc.size_slabs(n)] for n in range(jc.SIZE_RANGE)]
    assert all(len(jc.size_slabs(n)) == 4 for n in range(16, jc.SIZE_RANGE))  # (16: the first size a kernel serves)
    for answers in recorded["settings"].values():
        assert sorted(answers) == ["dts_bytes", "fold", "kernel", "packed_bytes", "run_as", "supported", "worksize"]
        assert all(len(v) == jc.SIZE_RANGE for v in answers.values())
    # the settings differ where they should: the file is not five copies of one table
    kernels = {s: a["kernel"] for s, a in recorded["settings"].items()}
    assert kernels[""][148] == jc.M8 and kernels["NBX_JK_M8=0"][148] == jc.M4
    assert kernels["NBX_JK_M8=0 NBX_JK_M4=0"][140] == jc.S4 and kernels["NBX_JK_MX=0"][152] == jc.S4
    assert kernels["NBX_JK_M4=0"][143] == jc.M8 and kernels["NBX_JK_M4=0"][144] == jc.MX


@pytest.mark.parametrize("setting", jc.SIZE_SETTINGS, ids=lambda s: s.replace(" ", ",") or "default")
def test_size_queries_answer_what_was_recorded(recorded, setting):
    want = recorded["settings"][setting]
    got = jc.packed_size_answers_in_child(setting)
    for query, values in want.items():
        bad = [(n, got[query][n], values[n]) for n in range(jc.SIZE_RANGE) if got[query][n] != values[n]]
        assert not bad, f"{query} under '{setting}': {len(bad)} sizes differ, first (n, got, recorded) {bad[:3]}"
