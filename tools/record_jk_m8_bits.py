"""Record tests/golden/jk_m8_bits.json: one SHA-256 of the raw output bytes per case of
tests/test_gpu_jk_m8_bookkeeping.py, computed on the library this process loads (NBX_LIB in the environment selects a
build other than the tree's: run it on a build of the commit whose bits are to be pinned).

    python tools/record_jk_m8_bits.py [OUT.json]      (default: tests/golden/jk_m8_bits.json)

Needs the MI355X.  The committed file was recorded on commit b416d28 (the one before M8Tables), with NBX_LIB pointing at a
libnbx.so built from it.  It only changes when a sum of jk_m8.hip changes its order or its terms: a change of where
the ranges' bookkeeping is computed or of how loads are batched must reproduce it."""

import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / "tests")]


def main():
    import test_gpu_jk_m8_bookkeeping as cases
    from nbed_amd.backend import HipBackend

    out = Path(sys.argv[1]) if len(sys.argv) > 1 else cases.GOLDEN_FILE
    be = HipBackend()
    bits = cases.all_bits(be)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(bits, indent=0, sort_keys=True) + "\n")
    print(f"{len(bits)} hashes -> {out}")


if __name__ == "__main__":
    main()
