"""The kernels' compile-time knobs: a short, documented list.

Every `#ifndef GSR_* / #define GSR_*` override under csrc/ is a variant that no test builds, so
the set is kept small on purpose: a new knob has to be added here and to DESIGN §8's table."""
import glob
import os
import re

from conftest import ROOT, pkg

CSRC = os.path.join(ROOT, "3d_gaussian_splatting_amd", "csrc")

# sizes and cut-over thresholds whose two sides both run in the suite at the default
KNOBS = {
    "GSR_CHUNK_WORK",
    "GSR_BAND_CHUNK_WORK",
    "GSR_MAX_CHUNKS",
    "GSR_PRESORT_MIN",
    "GSR_PRESORT_PER_TILE",
    "GSR_BLOCK8_TILES",
}


def source_knobs():
    """{macro: default} of every `#ifndef M` / `#define M default` pair under csrc/."""
    found = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "**", "*"), recursive=True)):
        if not path.endswith((".hip", ".h", ".cpp")):
            continue
        lines = open(path).read().split("\n")
        for i, line in enumerate(lines):
            m = re.match(r"\s*#\s*ifndef\s+(GSR_\w+)\s*$", line)
            if not m:
                continue
            d = re.match(r"\s*#\s*define\s+%s\s+(.*?)\s*$" % m.group(1), lines[i + 1])
            assert d, f"{path}:{i + 1}: #ifndef {m.group(1)} without its #define on the next line"
            assert m.group(1) not in found, f"{m.group(1)} defined twice"
            found[m.group(1)] = d.group(1)
    return found


def design_knobs():
    """{macro: default} from the knob table of DESIGN.md §8."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("\n## 8. Build"):]
    sec = sec[:sec.index("\n## ", 1)]
    rows = re.findall(r"^\| `(GSR_\w+)` \| `([^`]*)` \|", sec, re.M)
    assert rows, "DESIGN.md §8 has no knob table"
    return dict(rows)


def test_knob_set_is_the_documented_one():
    assert set(source_knobs()) == KNOBS


def test_knob_defaults_match_design():
    assert source_knobs() == design_knobs()


def test_build_lists_every_kernel_source():
    """build_hip compiles the HIP_SOURCES dict, build_variant whatever csrc/ holds: the same files."""
    on_disk = {f for f in os.listdir(CSRC) if f.endswith(".hip") or f in ("gsr_api.cpp", "gsr_comm.cpp")}
    assert on_disk == set(pkg("_build").HIP_SOURCES)


def test_build_passes_no_knob():
    b = pkg("_build")
    flags = list(b.COMMON) + [f for fl in b.HIP_SOURCES.values() for f in fl]
    assert not [f for f in flags if f.startswith("-DGSR_")]
