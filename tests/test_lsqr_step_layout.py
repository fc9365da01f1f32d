"""The ctypes mirrors of tests/lsqr_step.py against the C header (CPU only).

lsqr_step.py passes mspi_lsqr_dev by value and writes mspi_lsqr_state into device memory byte for byte; a mirror
that disagrees with msplit_internal.h would hand the kernels stray device pointers.  So the host C compiler says
what sizeof and every offsetof are, and the mirrors must agree before any of it runs on a GPU.  The twin of
tests/test_gmres_step_layout.py.
"""
import os
import re
import shutil
import subprocess

import pytest

import lsqr_step as ls
import lsqr_twin as lt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "medane_tchakorom_ufc_thesis_repository_amd", "csrc")
STRUCTS = (("mspi_lsqr_state", ls.STATE_INTS + ls.STATE_DOUBLES), ("mspi_lsqr_dev", ls.DEV_FIELDS))


def _program():
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "msplit_internal.h"', "int main(void) {"]
    for ctype, fields in STRUCTS:
        lines.append(f'  printf("{ctype} sizeof %zu\\n", sizeof({ctype}));')
        lines += [f'  printf("{ctype} {f} %zu\\n", offsetof({ctype}, {f}));' for f in fields]
    return "\n".join(lines + ["  return 0;", "}", ""])


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc")
    assert cc, "no host C compiler"
    d = tmp_path_factory.mktemp("lsqr_layout")
    src, exe = d / "layout.c", d / "layout"
    src.write_text(_program())
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC, str(src),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    out = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        ctype, field, value = line.split()
        out.setdefault(ctype, {})[field] = int(value)
    return out


@pytest.mark.parametrize("ctype,mirror", [("mspi_lsqr_state", ls.LsqrState), ("mspi_lsqr_dev", ls.LsqrDev)])
def test_mirror_matches_header(c_layout, ctype, mirror):
    """Same size, same fields in the same order at the same offsets."""
    want = c_layout[ctype]
    assert ls.layout(mirror) == want
    assert list(ls.layout(mirror)) == list(want)          # the program printed them in the mirror's order


def test_header_has_no_field_the_mirror_lacks():
    """A field added to either struct in the header must be added to the mirror: count the declarators."""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "msplit_internal.h")).read(), flags=re.S)
    for ctype, fields in STRUCTS:
        body = re.search(r"typedef struct \{([^}]*)\} " + ctype + ";", txt).group(1)
        names = re.findall(r"\*?\s*(\w+)\s*[,;]", body)
        assert tuple(names) == tuple(fields), ctype


def test_state_is_whole_doubles():
    """The state is pushed as doubles; its 12 32-bit fields come before the first double, which they leave
    8-byte aligned with no hole."""
    assert len(ls.STATE_INTS) == 12
    assert ls.layout(ls.LsqrState)["sizeof"] % 8 == 0
    assert ls.LsqrState.rnorm.offset == 4 * len(ls.STATE_INTS)
    assert ls.layout(ls.LsqrState)["sizeof"] == 4 * len(ls.STATE_INTS) + 8 * len(ls.STATE_DOUBLES)


def test_the_twin_state_has_the_mirror_fields():
    """tests/lsqr_twin.py's dict state is pushed field by field: it holds exactly the names of tests/lsqr_names.py,
    from which the mirror is built."""
    assert set(lt.new_state(3, 2)) == set(ls.STATE_INTS + ls.STATE_DOUBLES + ls.VECTORS)
