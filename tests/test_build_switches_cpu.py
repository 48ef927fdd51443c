"""Every compile-time switch of trep_amd/csrc is listed here and documented in DESIGN.md.

The kernel sources once carried some forty experiment switches nobody built; reading the Newton loop meant evaluating macros in one's
head.  This test keeps them from growing back: a new `#if` on a new name has to be added to ALLOWED below and described in DESIGN.md
before it lands.  It reads source text only.
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trep_amd", "csrc")

ALLOWED = {
    # product flags (trep_amd/specialize.py)
    "TG_GJ_INLINE", "SPEC_ARGS_IN_MEMORY", "SPEC_DERIVATIVES", "TG_HELPER_WAVES", "TG_SPEC_KEY", "TG_SPEC_HEADER",
    # set by spec_kernel.hip itself: what the specialised kernels have and the generic ones leave out
    "TG_GJ_PANEL_DEFAULT",
    # diagnostic instrumentation (`make prof`, tools/micro/bbd_bench.hip)
    "TG_PROFILE", "TG_PROF_TRAJ", "TG_BBD_STAMPS",
    # variants a GPU test builds and checks (test_packed_newton_image_and_item_form_variants)
    "TG_BBD_PACKED", "TG_NO_WEV",
    # compiler passes, and the discopt kernels' own tunable
    "__HIPCC__", "__HIP_DEVICE_COMPILE__", "LQM_THREADS",
}

_CONDITIONAL = re.compile(r"^\s*#\s*(if|ifdef|ifndef|elif)\b(.*)$")
_ERROR = re.compile(r"^\s*#\s*error\b")
_IDENT = re.compile(r"[A-Za-z_]\w*")


def _logical_lines(text):
    """Source lines with backslash continuations joined and comments dropped."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    lines, cur = [], ""
    for raw in text.split("\n"):
        raw = raw.split("//")[0].rstrip()
        if raw.endswith("\\"):
            cur += raw[:-1] + " "
            continue
        lines.append(cur + raw)
        cur = ""
    return [l for l in lines if l.strip()]


def _switches():
    """(tested, refused): the names the conditionals of csrc test, and the retired names of the one block of mvi_core.hpp that refuses
    them -- the first conditional of that file, directly followed by its #error.  No other conditional is exempt."""
    tested, refused = {}, {}
    files = sorted(f for f in glob.glob(os.path.join(CSRC, "*")) if os.path.isfile(f))
    assert len(files) >= 10, files
    for path in files:
        with open(path, errors="replace") as fh:
            lines = _logical_lines(fh.read())
        first = True
        for i, line in enumerate(lines):
            m = _CONDITIONAL.match(line)
            if not m:
                continue
            names = set(_IDENT.findall(m.group(2))) - {"defined"}
            guards_error = first and os.path.basename(path) == "mvi_core.hpp" and i + 1 < len(lines) and _ERROR.match(lines[i + 1])
            first = False
            for n in names:
                (refused if guards_error else tested).setdefault(n, set()).add(os.path.basename(path))
    return tested, refused


def test_every_build_switch_is_listed_and_documented():
    tested, refused = _switches()
    assert "__HIP_DEVICE_COMPILE__" in tested and "TG_PROFILE" in tested      # (the scan found the sources)
    assert "TG_MOCK_TIMING" in refused and "TG_NO_CMP" in refused             # (... and the block that refuses the retired names)
    unknown = {n: sorted(f) for n, f in tested.items() if n not in ALLOWED}
    assert not unknown, "compile-time switches that are neither listed in this test nor documented: %r" % unknown
    # a retired name may only stop the build; it must not come back as a switch under the same name
    assert not (set(refused) & ALLOWED), sorted(set(refused) & ALLOWED)
    assert not (set(refused) & set(tested)), sorted(set(refused) & set(tested))
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        design = fh.read()
    undocumented = sorted(n for n in ALLOWED if n.startswith(("TG_", "SPEC_")) and not re.search(r"\b%s\b" % n, design))
    assert not undocumented, "switches missing from DESIGN.md: %r" % undocumented
