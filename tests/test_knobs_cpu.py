"""The RLHIP_* environment knobs (ranklib_amd/csrc/rl_knobs.h): read in one file, named in one table.  Source text only: no GPU, no library."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ranklib_amd", "csrc")
KNOB = re.compile(r"RLHIP_[A-Z0-9_]+")
# names the host side reads (ranklib_amd/_native.py, bench.py, the tests' own workers), not the library
HARNESS = {"RLHIP_LIB", "RLHIP_BENCH_TRANSPORT", "RLHIP_BENCH_SAME_GPU", "RLHIP_TEST_JNI_STANDIN_H", "RLHIP_ABI_VERSION"}


def _read(path):
    with open(path, errors="replace") as f:
        return f.read()


def _header_knobs():
    return set(KNOB.findall(_read(os.path.join(CSRC, "rl_knobs.h"))))


def test_the_environment_is_read_in_rl_knobs_h_only():
    readers = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*")) if os.path.isfile(p) and "getenv" in _read(p))
    assert readers == ["rl_knobs.h"]


def test_the_design_table_names_exactly_the_knobs_of_the_header():
    design = _read(os.path.join(ROOT, "DESIGN.md"))
    start = design.index("Environment knobs")
    rows = [line for line in design[start:].splitlines() if line.startswith("| `RLHIP_")]
    names = [KNOB.search(line).group(0) for line in rows]
    assert len(names) == len(set(names)), "a knob has two rows"
    header = _header_knobs()
    assert header, "no knob found in rl_knobs.h"
    assert set(names) == header, (sorted(header - set(names)), sorted(set(names) - header))


def test_every_knob_a_test_sets_exists():
    used = set()
    for path in glob.glob(os.path.join(ROOT, "tests", "*.py")):
        if os.path.abspath(path) != os.path.abspath(__file__):
            used |= set(KNOB.findall(_read(path)))
    unknown = used - _header_knobs() - HARNESS
    assert not unknown, sorted(unknown)
