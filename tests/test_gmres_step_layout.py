"""The ctypes mirrors of tests/gmres_step.py against the C header (CPU only).

gmres_step.py passes mspi_gmres_dev by value and writes mspi_gmres_state into device memory byte for byte; a mirror
that disagrees with msplit_internal.h would hand the kernels stray device pointers.  So the host C compiler says
what sizeof and every offsetof are, and the mirrors must agree before any of it runs on a GPU.
"""
import os
import re
import shutil
import subprocess

import pytest

import gmres_step as gs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "medane_tchakorom_ufc_thesis_repository_amd", "csrc")


def _program():
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "msplit_internal.h"', "int main(void) {"]
    for ctype, fields in (("mspi_gmres_state", gs.STATE_INTS + gs.STATE_DOUBLES), ("mspi_gmres_dev", gs.DEV_FIELDS)):
        lines.append(f'  printf("{ctype} sizeof %zu\\n", sizeof({ctype}));')
        lines += [f'  printf("{ctype} {f} %zu\\n", offsetof({ctype}, {f}));' for f in fields]
    return "\n".join(lines + ["  return 0;", "}", ""])


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc")
    assert cc, "no host C compiler"
    d = tmp_path_factory.mktemp("layout")
    src, exe = d / "layout.c", d / "layout"
    src.write_text(_program())
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC, str(src),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    out = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        ctype, field, value = line.split()
        out.setdefault(ctype, {})[field] = int(value)
    return out


@pytest.mark.parametrize("ctype,mirror", [("mspi_gmres_state", gs.GmresState), ("mspi_gmres_dev", gs.GmresDev)])
def test_mirror_matches_header(c_layout, ctype, mirror):
    """Same size, same fields in the same order at the same offsets."""
    want = c_layout[ctype]
    assert gs.layout(mirror) == want
    assert list(gs.layout(mirror)) == list(want)          # the program printed them in the mirror's order


def test_header_has_no_field_the_mirror_lacks():
    """A field added to either struct in the header must be added to the mirror: count the declarators."""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "msplit_internal.h")).read(), flags=re.S)
    for ctype, fields in (("mspi_gmres_state", gs.STATE_INTS + gs.STATE_DOUBLES), ("mspi_gmres_dev", gs.DEV_FIELDS)):
        body = re.search(r"typedef struct \{([^}]*)\} " + ctype + ";", txt).group(1)
        names = re.findall(r"\*?\s*(\w+)\s*[,;]", body)
        assert tuple(names) == tuple(fields), ctype


def test_state_is_whole_doubles():
    """The state is pushed as doubles and its 32-bit fields come in pairs before the first double."""
    assert gs.layout(gs.GmresState)["sizeof"] % 8 == 0
    assert gs.GmresState.res.offset == 4 * len(gs.STATE_INTS)
