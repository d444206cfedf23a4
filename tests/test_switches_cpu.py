"""The inventory of MHIMX_* environment switches: the package reads exactly the ones DESIGN.md section 5 lists, and the C side reads none
(a `static const` getenv is read once per process, so no test could ever flip it: a form that is worth keeping gets a Python switch or an
argument, a form that lost is deleted)."""
import pathlib
import re

PKG = pathlib.Path(__file__).resolve().parents[1] / "mhim_mil_amd"

AB_SWITCHES = {"MHIMX_STEP_EXEC", "MHIMX_STEP_DAG", "MHIMX_WINDOW_BATCHED", "MHIMX_WINDOW_PROJECT", "MHIMX_WINDOW_WGRAD", "MHIMX_PINV_CHAIN",
               "MHIMX_PINV_LEVELS", "MHIMX_TOKENS_NODE", "MHIMX_STEP_IMAGES", "MHIMX_PPEG_BAND_W1"}
BUILD_PLUMBING = {"MHIMX_LIB_NAME", "MHIMX_EXTRA_FLAGS"}


def test_the_environment_switches_are_the_documented_ten():
    found = set()
    for f in PKG.rglob("*.py"):
        found |= set(re.findall(r"""os\.environ(?:\.get\(|\.setdefault\(|\[)\s*["'](MHIMX_\w+)""", f.read_text()))
    csrc = [f for f in (PKG / "csrc").iterdir() if f.is_file()]
    assert csrc
    for f in csrc:
        text = f.read_text()
        found |= set(re.findall(r"""getenv\(\s*"(MHIMX_\w+)""", text))
        assert "getenv" not in text, f"{f.name} reads the environment"
    assert found == AB_SWITCHES | BUILD_PLUMBING, (sorted(found - AB_SWITCHES - BUILD_PLUMBING), sorted((AB_SWITCHES | BUILD_PLUMBING) - found))
