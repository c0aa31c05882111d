"""The engine's Makefile rebuilds every object that reaches an edited header, .inc body or included source (no GPU, no compiler).

bayhunter_amd/csrc/Makefile keeps no list of header prerequisites: the compiler writes them beside every object as it compiles
(-MMD -MP) and the next run reads them.  This test holds that to the sources themselves.  It follows the quoted #include lines of
every unit of SRC textually -- it does not read the .d files -- and asks `make -n -W <file>` ("as if <file> had just been edited")
for every project header and included source: the dry run must name the compile of every object whose source reaches the file.

It runs after the build (the dependency files come from it).  In a tree with no objects every dry run names every compile, which
is right as well: there is nothing stale to keep.
"""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "bayhunter_amd", "csrc")
INCLUDE = os.path.join(REPO, "include")

# (unit, file) pairs whose #include sits under a condition that the unit's build turns off, with the condition: the textual walk
# reaches the file, the compiler does not.  There is none today: no quoted #include of the tree stands under #if / #ifdef.
CONDITIONAL = {
}

_INCLUDE_LINE = re.compile(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', re.M)


def _units():
    with open(os.path.join(CSRC, "Makefile")) as f:
        return re.search(r"^SRC\s*:=\s*(.*)$", f.read(), re.M).group(1).split()


def _reached(path, seen):
    """every file that `path` reaches through quoted #include lines (resolved beside the including file, as the compiler does)"""
    with open(path) as f:
        names = _INCLUDE_LINE.findall(f.read())
    for name in names:
        q = os.path.normpath(os.path.join(os.path.dirname(path), name))
        assert os.path.isfile(q), "%s includes \"%s\": no such file" % (os.path.relpath(path, REPO), name)
        if q not in seen:
            seen.add(q)
            _reached(q, seen)
    return seen


@pytest.fixture(scope="module")
def reach():
    """unit -> the set of files its source reaches"""
    return {u: _reached(os.path.join(CSRC, u), set()) for u in _units()}


def _compiles_named(edited):
    """the objects whose compile `make -n -W edited` names"""
    rel = os.path.relpath(edited, CSRC)
    out = subprocess.run(["make", "-C", CSRC, "-n", "-W", rel], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
    return set(re.findall(r"-c \S+\.hip -o (\S+\.o)\b", out))


def test_every_object_that_reaches_a_file_is_rebuilt_with_it(reach):
    units = _units()
    included_sources = {f for fs in reach.values() for f in fs if f.endswith(".hip")}
    files = sorted({os.path.join(CSRC, n) for n in os.listdir(CSRC) if n.endswith((".h", ".inc"))}
                   | {os.path.join(INCLUDE, n) for n in os.listdir(INCLUDE) if n.endswith(".h")} | included_sources)
    assert len(files) > 40 and len(units) > 40 and included_sources  # (the walk found the tree)
    stale = []
    for f in files:
        want = {u[:-4] + ".o" for u in units if f in reach[u] and (u, os.path.relpath(f, REPO)) not in CONDITIONAL}
        if not want:
            continue
        missing = want - _compiles_named(f)
        if missing:
            stale.append("%s: not rebuilt: %s" % (os.path.relpath(f, REPO), " ".join(sorted(missing))))
    assert not stale, "an edit of these files leaves stale objects in the library:\n" + "\n".join(stale)


def test_conditional_pairs_are_reached_textually(reach):
    for (unit, rel), why in CONDITIONAL.items():
        assert why and os.path.join(REPO, rel) in reach[unit], (unit, rel)


def test_makefile_lists_no_header_by_hand():
    with open(os.path.join(CSRC, "Makefile")) as f:
        rules = [l for l in f.read().split("\n") if re.match(r"^[^#\t][^=]*:(?!=)", l)]
    assert rules
    by_hand = [l for l in rules if re.search(r"\.(h|inc)\b", l.split(":", 1)[1]) or re.search(r"\.o\b.*:.*\.hip\b", l) and not l.startswith("%")]
    assert not by_hand, by_hand
