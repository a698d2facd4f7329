"""The ctypes mirrors of smhip_guess_search_options / smhip_guess_search_result (staticmapping_amd/_capi.py) against include/smhip.h, the
way tests/test_capi_layout.py checks the older structs: a C program prints sizes and offsets; and the defaults the library hands out."""
import ctypes
import math
import os
import subprocess

import pytest

from staticmapping_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [("smhip_guess_search_options", _capi.GuessSearchOptions), ("smhip_guess_search_result", _capi.GuessSearchResult)]


@pytest.mark.parametrize("cname,cls", PAIRS)
def test_ctypes_mirror_has_the_headers_layout(tmp_path, cname, cls):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "smhip.h"', "int main(void) {", f'  printf("size %zu\\n", sizeof({cname}));']
    for fname, _ in cls._fields_:
        lines.append(f'  printf("{fname} %zu %zu\\n", offsetof({cname}, {fname}), sizeof((({cname}*)0)->{fname}));')
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    want = {ln.split()[0]: tuple(int(v) for v in ln.split()[1:]) for ln in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines()}
    assert ctypes.sizeof(cls) == want["size"][0]
    covered = 0
    for fname, ftype in cls._fields_:
        off, size = want[fname]
        assert getattr(cls, fname).offset == off and ctypes.sizeof(ftype) == size, fname
        covered = max(covered, off + size)
    assert want["size"][0] - covered < 8


def test_defaults():
    from staticmapping_amd import build, guess_search
    build.build()
    o = guess_search.make_options()
    assert (o.resolution, o.max_source_points, o.half_xy, o.half_z, o.yaw_steps, o.reserved) == (0.5, 4096, 20, 2, 10, 0)
    assert o.yaw_step == 2.0 * math.pi / 180.0
    assert guess_search.make_options(half_xy=3, resolution=0.25).half_xy == 3
    with pytest.raises(TypeError):
        guess_search.make_options(window=3)
