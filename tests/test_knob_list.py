"""The environment switches of libnps_hip.so are exactly the ones INTEGRATION.md lists: every NPS_* name the
library's sources read (through nps::env_flag, nps_common.hpp — or a bare getenv, which is how dev knobs crept in
before) against the "Library switches" paragraph.  A new switch has to be documented there, and so argued for."""
import pathlib
import re

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "neural-pde-surrogates_amd" / "csrc"
NAME = re.compile(r'"(NPS_[A-Z0-9_]+)"')
READER = re.compile(r"\b(getenv|env_flag)\s*\(")


def _sources():
    return sorted(list(CSRC.glob("*.hip")) + list(CSRC.glob("*.hpp")))


def _documented():
    paras = [p for p in (ROOT / "INTEGRATION.md").read_text().split("\n\n") if p.startswith("**Library switches**")]
    assert len(paras) == 1, "INTEGRATION.md: one paragraph starting with **Library switches**"
    return set(re.findall(r"`(NPS_[A-Z0-9_]+)(?:=[^`]*)?`", paras[0]))


def test_library_env_switches_are_the_documented_ones():
    read = {}
    for f in _sources():
        for n, line in enumerate(f.read_text().splitlines(), 1):
            if READER.search(line):
                for name in NAME.findall(line):
                    read.setdefault(name, []).append(f"{f.name}:{n}")
    assert read, "found no switch at all: the scan is broken"
    doc = _documented()
    assert set(read) == doc, (f"read but not in INTEGRATION.md: {sorted((k, read[k]) for k in set(read) - doc)}; "
                              f"documented but not read: {sorted(doc - set(read))}")


def test_getenv_only_in_the_helper():
    """A getenv whose name is not a literal on the same line would escape the scan above: only env_flag may call it."""
    calls = [f"{f.name}:{n}" for f in _sources() for n, line in enumerate(f.read_text().splitlines(), 1)
             if re.search(r"\bgetenv\s*\(", line)]
    assert len(calls) == 1 and calls[0].startswith("nps_common.hpp:"), calls
