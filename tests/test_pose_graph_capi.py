"""The pose graph's C ABI without a GPU: the ctypes mirrors of smhip_pose_graph_options / _stats against the header's layout (as
test_capi_layout.py does for the other structs), and smhip_pose_graph_plan -- the host half of smhip_pose_graph_optimize -- through
staticmapping_amd.pose_graph.plan: the CSR list in edge order and the refusals with their reasons."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pose_graph_cases as cases
from staticmapping_amd import _capi, pose_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [("smhip_pose_graph_options", _capi.PoseGraphOptions), ("smhip_pose_graph_stats", _capi.PoseGraphStats)]


@pytest.mark.parametrize("cname,cls", PAIRS)
def test_ctypes_mirror_has_the_headers_layout(tmp_path, cname, cls):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "smhip.h"', "int main(void) {", f'  printf("size %zu\\n", sizeof({cname}));']
    for fname, _ in cls._fields_:
        lines.append(f'  printf("{fname} %zu %zu\\n", offsetof({cname}, {fname}), sizeof((({cname}*)0)->{fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)], check=True)
    want = {ln.split()[0]: tuple(int(x) for x in ln.split()[1:]) for ln in
            subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines()}
    assert ctypes.sizeof(cls) == want["size"][0]
    covered = 0
    for fname, ftype in cls._fields_:
        off, size = want[fname]
        assert getattr(cls, fname).offset == off and ctypes.sizeof(ftype) == size, fname
        covered = max(covered, off + size)
    assert want["size"][0] - covered < 8
    assert (pose_graph.MAX_NODES, pose_graph.MAX_EDGES) == (8192, 32768)
    hdr = open(os.path.join(ROOT, "include", "smhip.h")).read()
    assert "#define SMHIP_POSE_GRAPH_MAX_NODES 8192" in hdr and "#define SMHIP_POSE_GRAPH_MAX_EDGES 32768" in hdr


def test_plan_lists_every_nodes_edges_in_index_order():
    g = cases.stage_cases()["reversed_and_double"]
    off, inc = pose_graph.plan(g["poses"], g["edges"], g["Z"], fixed=g["fixed"])
    assert off[0] == 0 and off[-1] == 2 * len(g["edges"])
    for k in range(len(g["poses"])):
        mine = inc[off[k]:off[k + 1]]
        assert list(mine) == [e for e, (i, j) in enumerate(g["edges"]) if k in (i, j)]


def test_plan_refuses_with_a_reason():
    g = cases.stage_cases()["n5"]

    def refused(status, word, **change):
        with pytest.raises(pose_graph.PoseGraphRefused, match=word) as err:
            pose_graph.plan(**{**dict(poses=g["poses"], edges=g["edges"], Z=g["Z"], fixed=g["fixed"]), **change})
        assert err.value.status == status
    invalid, capacity = 1, 7
    e = g["edges"].copy()
    e[2] = (2, 9)
    refused(invalid, "out of range", edges=e)
    e = g["edges"].copy()
    e[2] = (3, 3)
    refused(invalid, "itself", edges=e)
    refused(invalid, "sigma", sigmas=[0.1, 0.1, 0.0, 0.15, 0.15, 0.15])
    refused(invalid, "sigma", sigmas=[0.1, 0.1, np.nan, 0.15, 0.15, 0.15])
    p = g["poses"].copy()
    p[2, 1, 3] = np.nan
    refused(invalid, "pose 2 is not finite", poses=p)
    p = g["poses"].copy()
    p[4, :3, :3] *= 1.00001
    refused(invalid, "pose 4 .*orthonormal", poses=p)
    z = g["Z"].copy()
    z[1, :3, 0] *= -1.0
    refused(invalid, "edge 1's measurement .*reflection", Z=z)
    refused(invalid, "no fixed node", fixed=np.zeros(5, np.uint8))
    refused(invalid, "free node 4 has no edge", edges=g["edges"][[0, 1, 2, 5]], Z=g["Z"][[0, 1, 2, 5]])
    big = np.tile(np.eye(4), (pose_graph.MAX_NODES + 1, 1, 1))
    chain = np.stack([np.arange(pose_graph.MAX_NODES), np.arange(1, pose_graph.MAX_NODES + 1)], axis=1)
    refused(capacity, "8192 nodes", poses=big, edges=chain, Z=np.tile(np.eye(4), (len(chain), 1, 1)), fixed=None)
    many = np.tile([[0, 1]], (pose_graph.MAX_EDGES + 1, 1))
    refused(capacity, "32768 edges", poses=big[:2], edges=many, Z=np.tile(np.eye(4), (len(many), 1, 1)), fixed=None)
    # at the limits: accepted
    off, inc = pose_graph.plan(big[:-1], chain[:-1], np.tile(np.eye(4), (len(chain) - 1, 1, 1)))
    assert off[-1] == 2 * (pose_graph.MAX_NODES - 1)
