"""Record tests/golden/settled_trips_bits.json: one SHA-256 of the raw output bytes per case of
tests/test_gpu_settled_trips.py, computed on the library this process loads (NBX_LIB in the environment selects a
build other than the tree's: run it on a build of the commit whose bits are to be pinned).

    python tools/record_settled_bits.py [OUT.json]      (default: tests/golden/settled_trips_bits.json)

Needs the MI355X.  The file only changes when a kernel's arithmetic does: a change of how loads are batched, waves
are assigned or launches are scheduled must reproduce it."""

import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / "tests")]


def main():
    import test_gpu_settled_trips as cases
    from nbed_amd.backend import HipBackend

    out = Path(sys.argv[1]) if len(sys.argv) > 1 else cases.GOLDEN_FILE
    be = HipBackend()
    bits = cases.all_bits(be)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(bits, indent=0, sort_keys=True) + "\n")
    print(f"{len(bits)} hashes -> {out}")


if __name__ == "__main__":
    main()
