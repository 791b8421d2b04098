"""The boundary between bindings.cpp and the kernel files is declared once.

``extern "C"`` symbols are not mangled: a caller's declaration that disagrees
with the definition links cleanly and runs with shifted arguments. So every
entry point is declared in ``csrc/launchers.h`` alone, every ``.hip`` file
and ``bindings.cpp`` include it, and the compiler then rejects a definition
or call that disagrees. These tests keep that layout from eroding; they read
source text only and need no GPU.
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpi_operator_amd", "ops", "csrc")


def _code(path):
    """File text without comments (they may speak of extern "C")."""
    with open(path, encoding="utf-8") as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip"))) + [
        os.path.join(CSRC, "bindings.cpp")]


def _extern_c_items(code):
    """(text up to the first ';' or '{', that terminator) per extern "C"."""
    return re.findall(r'extern\s+"C"\s*([^;{]*)([;{])', code)


def test_every_translation_unit_includes_launchers_h():
    assert len(_sources()) >= 12
    for path in _sources():
        assert re.search(r'^#include "launchers\.h"', _code(path), re.M), path


def test_extern_c_is_declared_only_in_launchers_h():
    for path in glob.glob(os.path.join(CSRC, "*")):
        if os.path.basename(path) == "launchers.h":
            continue
        decls = [head.strip() for head, end in _extern_c_items(_code(path))
                 if end == ";"]
        assert not decls, (path, decls)


def test_every_extern_c_definition_is_declared_in_launchers_h():
    header = _code(os.path.join(CSRC, "launchers.h"))
    defined = []
    for path in glob.glob(os.path.join(CSRC, "*.hip")):
        for head, end in _extern_c_items(_code(path)):
            m = re.search(r"(\w+)\s*$", head.split("(")[0])
            assert m and end == "{", (path, head)
            defined.append(m.group(1))
    assert len(defined) > 60  # the parser found the entry points
    missing = [n for n in defined if not re.search(r"\b%s\s*\(" % n, header)]
    assert not missing, missing


def test_descriptor_structs_are_defined_once():
    text = "".join(_code(p) for p in glob.glob(os.path.join(CSRC, "*")))
    for name in ("SgdDesc", "OptDesc"):
        assert len(re.findall(r"\bstruct\s+%s\b" % name, text)) == 1, name
