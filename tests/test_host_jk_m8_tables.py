"""M8Tables of csrc/jk_m8.hip -- where each workgroup's range of tiles starts, made on the host beside M8Ranges::first
and read by jk_m8_kernel instead of being computed in every wave -- on EVERY row slab of three instances (the smallest,
a middle one, the benchmark's), without a GPU: tests/native/m8_tables_check.hip runs m8_ranges itself, whose own
comparison with m8_tile_offset / m8_tri_row must report nothing, and checks cover, order and ranges on top.  The host
code is built with AddressSanitizer and UBSan (a stand-alone program: the sanitizers see m8_ranges' writes into the
tables); three instances keep the compile to seconds."""

import shutil
import subprocess
from pathlib import Path

import pytest

from nbed_amd import _nbx

ROOT = Path(__file__).resolve().parent.parent
SIZES = (25, 31, 37)  # N = 100, 124, 148


def test_m8_tables_on_every_slab(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("no hipcc")
    lib = Path(_nbx.LIB_PATH)
    assert lib.exists(), "build() first: the check links libnbx.so"
    exe = tmp_path / "m8_tables_check"
    sizes = "-DNBX_M8_SIZES(X)=" + " ".join(f"X({nb})" for nb in SIZES)
    subprocess.run([hipcc, "-std=c++17", "-O1", "-g", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", sizes, f"-I{ROOT / 'include'}",
                    f"-I{ROOT / 'nbed_amd' / 'csrc'}", "-Wno-unused-function", "-Wno-inline-asm",
                    str(ROOT / "tests" / "native" / "m8_tables_check.hip"), "-o", str(exe), f"-L{lib.parent}", "-lnbx",
                    f"-Wl,-rpath,{lib.parent}"], check=True, capture_output=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for nb in SIZES:
        n = 4 * nb
        assert f"N={n}: {n * (n + 1) // 2} slabs, bad=0" in r.stdout, r.stdout
