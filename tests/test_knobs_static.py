"""Static checks of the library's environment switches.  No GPU needed.

The library reads the environment in one place only (the `jch_knob` / `jch_knob_set` helpers), every switch it consults is
documented in the table of surviving switches, and no retired switch has come back."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jchemo.jl_amd", "csrc")

KNOB_CALL = re.compile(r'\bjch_knob(?:_set)?\(\s*"(JCH_\w+)"')


def _sources():
    for name in sorted(os.listdir(CSRC)):
        path = os.path.join(CSRC, name)
        if os.path.isfile(path):
            with open(path, encoding="utf-8") as f:
                yield name, f.read()


def _table_names(part):
    """`JCH_*` names in the first column of the table rows of a piece of DESIGN.md."""
    first_cells = [ln.split("|")[1] for ln in part.splitlines() if ln.startswith("| `JCH_")]
    return set(re.findall(r"`(JCH_\w+)", "\n".join(first_cells)))


def _design_5c():
    with open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8") as f:
        text = f.read()
    beg = text.index("## 5c. Environment switches")
    mid = text.index("### Retired switches", beg)
    end = text.index("\n## ", mid)
    return _table_names(text[beg:mid]), _table_names(text[mid:end])


def test_getenv_only_in_the_helper():
    users = [name for name, text in _sources() if "getenv" in text]
    assert users == ["ctx.hip"], users
    helper = dict(_sources())["ctx.hip"]
    assert helper.count("getenv") == 2 and "jch_knob_set" in helper       # one call in each of the two helpers


def test_no_switch_cached_in_a_static():
    cached = re.compile(r"static (const )?(int|bool) \w+ = (-1|\[\]|getenv)")
    hits = [(name, m.group(0)) for name, text in _sources() for m in cached.finditer(text)]
    assert not hits, hits


def test_every_switch_read_is_a_documented_survivor():
    read = {}
    for name, text in _sources():
        for knob in KNOB_CALL.findall(text):
            read.setdefault(knob, name)
    surviving, retired = _design_5c()
    assert len(read) >= 20, read                                          # the pattern still finds the call sites
    undocumented = {k: v for k, v in read.items() if k not in surviving}
    assert not undocumented, undocumented
    assert not surviving & retired, surviving & retired
    # a retired name may still be spoken of in a comment, but nothing in csrc/ may pass one to the helpers
    assert not set(read) & retired, set(read) & retired
