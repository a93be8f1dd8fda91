"""
The include graph of csrc/ (header map at the top of csrc/lpc_engine.h), checked with g++ on the emulator's view of the
sources: every header stands on its own, and the units that launch nothing see no kernel.
"""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lenslesspicam_amd", "csrc")
GXX = ["g++", "-std=c++17", "-DLPC_SIMT_EMU", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-x", "c++"]
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".h"))
HOST_ONLY = ("lpc_abi.cpp", "lpc_planner.cpp", "lpc_jit.cpp")


@pytest.mark.parametrize("flavour", [[], ["-DLPC_DOUBLE"]], ids=["f32", "f64"])
def test_every_header_compiles_on_its_own(flavour):
    """a one-line source that includes the header and nothing else: no header leans on what its includer included"""
    def check(h):
        r = subprocess.run(GXX + flavour + ["-fsyntax-only", "-"], input=f'#include "{h}"\n', text=True,
                           capture_output=True)
        return h, r.returncode, r.stderr
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        bad = [(h, err[-2000:]) for h, rc, err in pool.map(check, HEADERS) if rc != 0]
    assert len(HEADERS) >= 18 and not bad, bad


def kernels_seen(unit):
    names = set()
    for h in HEADERS:
        names |= set(re.findall(r"void (k_\w+)\(", open(os.path.join(CSRC, h)).read()))
    assert len(names) > 50, names
    out = subprocess.run(GXX + ["-E", os.path.join(CSRC, unit)], text=True, capture_output=True, check=True).stdout
    return names & set(re.findall(r"\bk_\w+", out))


def test_host_only_units_see_no_kernel():
    """lpc_abi.cpp, lpc_planner.cpp and lpc_jit.cpp launch nothing: their preprocessed text names no kernel of any
    header.  (lpc_rows.cpp shows that the search finds kernels where there are some.)"""
    assert len(kernels_seen("lpc_rows.cpp")) > 10
    for unit in HOST_ONLY:
        assert kernels_seen(unit) == set(), unit
