"""The 2D-DWT's kernel schedule is a per-call argument: no environment reads and
no process-wide switches in the product library, and the one
band-cut model of its launchers (csrc/vcf_band_cut.h, built for the host with
g++) keeps the cuts of config C3 that its three earlier copies made."""
import ctypes
import glob
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "vcf_amd", "csrc")
# the product library's environment reads, all of them
GETENV_ALLOWED = {("vcf_png.cpp", "VCF_PNG_NO_LIBDEFLATE"), ("vcf_comm.cpp", "VCF_COMM_TIMEOUT_MS")}
# the product sources' compile-time switches, all of them: two instruments of the deflate, the
# inflate's window-check build (csrc/ab/vcf_inflate_wincheck.hip), the DWT kernels alone (scripts/micro/)
SWITCHES_ALLOWED = {"VCF_ZLIB_PROF", "VCF_ZX_WINCHECK", "VCF_INFLATE_WINCHECK_BUILD", "VCF_DWT_KERNELS_ONLY"}


def test_product_sources_read_no_other_environment():
    found = []
    for ext in ("hip", "h", "cpp"):
        for path in sorted(glob.glob(os.path.join(CSRC, "*." + ext))):   # (csrc/ab/, the A/B library, is not the product)
            src = open(path, errors="replace").read()
            for m in re.finditer(r"getenv\(\s*(\"(\w+)\")?", src):
                found.append((os.path.basename(path), m.group(2)))
    assert sorted(found) == sorted(GETENV_ALLOWED), found


def test_product_sources_have_no_other_compile_time_switch():
    """A measured and decided A/B leaves one form in the product sources, not a macro with both:
    every VCF_ name a preprocessor conditional tests (an `#ifndef VCF_X` / `#define VCF_X <default>`
    pair among them), include guards aside, is on the list."""
    found = set()
    paths = [p for ext in ("hip", "h", "cpp") for p in glob.glob(os.path.join(CSRC, "*." + ext))]
    for path in sorted(paths + glob.glob(os.path.join(ROOT, "include", "*.h"))):
        src = re.sub(r"/\*.*?\*/", "", open(path, errors="replace").read(), flags=re.S)
        src = re.sub(r"//[^\n]*", "", src)
        guards = set(re.findall(r"^[ \t]*#[ \t]*ifndef[ \t]+(\w+)[ \t]*\n[ \t]*#[ \t]*define[ \t]+\1[ \t]*$", src, flags=re.M))
        for line in re.findall(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b(.*)$", src, flags=re.M):
            found |= set(re.findall(r"\bVCF_\w+", line)) - guards
    assert found == SWITCHES_ALLOWED, sorted(found ^ SWITCHES_ALLOWED)


def test_removed_switches_are_gone():
    """The decided switches' names, anywhere a build could still set them: the DWT's second build,
    the two small A/B macros, and every VCF_ZX_ macro of the deflate but its window check."""
    hits = []
    for sub in (os.path.join("vcf_amd", "csrc"), "include", "scripts"):
        for dirpath, _, names in os.walk(os.path.join(ROOT, sub)):
            for name in sorted(names):
                path = os.path.join(dirpath, name)
                src = open(path, errors="replace").read()
                pat = r"VCF_DWT_SCHED_BUILD|VCF_B21_SPLIT|VCF_SDWA_ASM"
                if sub.endswith("csrc"):
                    pat += r"|VCF_ZX_(?!WINCHECK\b)\w+"
                hits += [(os.path.relpath(path, ROOT), m) for m in re.findall(pat, src)]
    assert not hits, hits


def test_public_header_has_no_kernel_setter():
    """No entry of the product ABI switches a kernel for the process: the declared names with `set`
    in them are the device, a fill, and the deflate workspace budget (a per-device resource)."""
    src = open(os.path.join(ROOT, "include", "vcf_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(vcf_\w*set\w*)\s*\(", src))) == ["vcf_memset", "vcf_set_device",
                                                                      "vcf_zlib_set_workspace_budget"]


def test_product_library_exports_no_kernel_setter():
    """The two process-wide switches it once had (names in two pieces: a search of the tree for them
    should find callers, not this test)."""
    import vcf_amd._lib as L
    for name in ("vcf_cbaac_tiled_set" "_variant", "vcf_ipp_set" "_full_search_variant"):
        assert not hasattr(L.lib(), name), name


@pytest.fixture(scope="module")
def band_cut(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("bc") / "band_cut_harness.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpu", "band_cut_harness.cpp"), "-o", so], check=True)
    f = ctypes.CDLL(so).bc_band_cut
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_int]
    f.restype = ctypes.c_int
    return f


# Config C3: 8 frames of 2160 x 3840, 5 levels -- subbands 1080 x 1920, 540 x 960, 270 x 480, 135 x 240,
# 68 x 120.  (rows, max_bands, per_band, steps_per_row, overhead) of every banded launch, as the launchers
# of vcf_dwt.hip pass them, and the bands at 512 and at 1024 resident workgroups.
C3_CUTS = [
    # encode levels 1 + 2: h2 = 540 rows, at most h2 / 2 bands, 3 x 8 frames x ceil(960 / 120) tiles
    ("band12", (540, 270, 192, 2, 13), 8, 5),
    # inverse line levels 5, 4, 3: ceil(h_{r-1} / 2) output row pairs, 8 frames x ceil(w_r / 64) tiles
    ("line 5", (68, 68, 16, 1, 5), 23, 34),
    ("line 4", (135, 135, 32, 1, 5), 15, 27),
    ("line 3", (270, 270, 64, 1, 5), 8, 16),
    # lifting level pairs 1 + 2 / 2 + 1 and 3 + 4 / 4 + 3: 8 frames x ceil(w / 58) strips
    ("lift pair 540", (540, 540, 136, 2, 12), 7, 7),
    ("lift pair 135", (135, 135, 40, 2, 12), 12, 23),
    # lifting level 5 alone: 8 frames x ceil(120 / 124) strips
    ("lift single", (68, 68, 8, 1, 4), 34, 68),
]


@pytest.mark.parametrize("what,args,at512,at1024", C3_CUTS, ids=[c[0] for c in C3_CUTS])
def test_band_cut_of_c3(band_cut, what, args, at512, at1024):
    rows, max_bands, per_band, steps, overhead = args
    assert band_cut(rows, max_bands, per_band, 512, steps, overhead) == at512
    assert band_cut(rows, max_bands, per_band, 1024, steps, overhead) == at1024

