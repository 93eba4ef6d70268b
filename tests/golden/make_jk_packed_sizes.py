"""Record what the host-arithmetic size queries of the packed J/K answer: tests/golden/jk_packed_sizes.json.

    python tests/golden/make_jk_packed_sizes.py <commit the built library comes from>

For every n in 0 .. 420 and every setting of tests/jk_cases.SIZE_SETTINGS (a child process each: the switches are read
once per process): nbx_jk_packed_supported, nbx_jk_packed_fold, nbx_jk_packed_route, nbx_jk_dts_bytes, and
nbx_eri_packed_bytes / nbx_jk_packed_worksize over the whole tensor and the slabs of jk_cases.equal_work_cuts.  No GPU
and no context are needed.

The file pins the answers of the library as it was BEFORE the dispatcher of csrc/jk_packed.hip replaced the hand-written
cascades (the commit is recorded in the file); tests/test_host_jk_packed_sizes.py holds every later library to them.
It is never regenerated from the code under test: a change of these numbers is a change of the packed buffers' sizes
(NBX_VERSION) and is made on purpose, with this file rewritten from a library that is known to be right.
"""

from __future__ import annotations

import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))
sys.dont_write_bytecode = True

import jk_cases as jc  # noqa: E402


def main():
    commit = sys.argv[1]
    out = {"commit": commit, "n": [0, jc.SIZE_RANGE - 1],
           "slabs": [jc.size_slabs(n) for n in range(jc.SIZE_RANGE)],
           "settings": {s: jc.packed_size_answers_in_child(s) for s in jc.SIZE_SETTINGS}}
    text = json.dumps(out, separators=(",", ":")) + "\n"
    assert len(text) < 1_000_000, len(text)
    (HERE / "jk_packed_sizes.json").write_text(text)
    print("wrote", len(text), "bytes for", len(out["settings"]), "settings")


if __name__ == "__main__":
    main()
