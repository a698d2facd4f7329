"""Known answers of the CPU restatement of GroundRemoval, GroundRemoval2 and RangeImage (tests/ground_filters_ref.py), the
constructor defaults and slot layout of the extended C descriptor, and the opt-in XML parse.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ground_filters_ref as gf
from staticmapping_amd import _capi, filters as df, synth
from oracle import filters as of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def rows(xyz) -> np.ndarray:
    a = np.zeros((len(xyz), 5), F)
    a[:, :3] = np.asarray(xyz, F)
    return a


def polar(d, az_deg, z) -> list:
    a = np.deg2rad(az_deg)
    return [d * np.cos(a), d * np.sin(a), z]


# ---- GroundRemoval2 ------------------------------------------------------------------------------------------------------
def test_membership_follows_the_running_minimum():
    pts = rows([polar(10.2, 5.0, z) for z in (0.0, 0.4, -0.3, 0.3)])
    grid, rng, z = gf.gr2_bin(pts, gf.gr2_params())
    assert len(set(grid.tolist())) == 1
    member, gmin = gf.gr2_grids(grid, rng, z)
    assert member.tolist() == [True, True, True, False]      # 0.4 joins against the minimum so far (0.0), 0.3 against -0.3
    assert gmin[grid[0]][1] == F(-0.3)


def test_points_inside_r_min_are_still_binned():
    pts = rows([polar(0.5, 30.0, -1.0), polar(150.0, 30.0, -1.0), [0.0, 0.0, -1.0]])
    grid, _, _ = gf.gr2_bin(pts, gf.gr2_params())
    assert (grid >= 0).all()
    assert grid[0] % 200 == 0 and grid[1] % 200 == 199 and grid[2] == 0   # clamped into the first / last bin


def _ground_ray(az, z0=-1.73, wobble=0.01):
    return [polar(d, az, z0 + wobble * np.sin(3.0 * d)) for d in np.arange(2.0, 40.0, 0.5)]


def test_neighbour_segment_search():
    p = dict(start_ground_height=-1.73)
    probe = polar(20.25, 11.0, -1.70)                         # segment 5 (2 degree segments): no line of its own
    pts = rows(_ground_ray(9.0) + [probe])
    keep = gf.ground_removal2(pts, **p)
    assert not keep[-1]                                       # found on segment 4's line, 0 < distance <= 0.05
    assert gf.ground_removal2(pts, search_angle=0.0, **p)[-1]  # no search: no line, kept
    far = rows(_ground_ray(9.0) + [polar(20.25, 25.0, -1.70)])  # 8 segments away: beyond search_angle 10
    assert gf.ground_removal2(far, **p)[-1]


def test_distance_of_exactly_zero_is_kept():
    flat = [polar(d, 45.0, -1.5) for d in np.arange(2.0, 30.0, 0.5)]
    pts = rows(flat + [polar(10.25, 45.0, -1.49)])
    keep = gf.ground_removal2(pts, start_ground_height=-1.5)
    lines = gf.gr2_fit_lines(gf.gr2_grids(*gf.gr2_bin(pts, gf.gr2_params()))[1], 22, gf.gr2_params(start_ground_height=-1.5))
    assert len(lines) >= 1 and (lines[:, 1] == F(-1.5)).all()
    assert keep[:-1].all()                                    # on the line: distance 0, kept
    assert not keep[-1]                                       # 0.01 above it: removed


def test_segment_with_data_only_in_its_last_bin():
    p = gf.gr2_params()
    pts = rows([polar(d, 91.0, -1.7) for d in (120.0, 130.0, 140.0, 150.0)])   # all beyond r_max: bin 199
    grid, rng, z = gf.gr2_bin(pts, p)
    assert (grid % 200 == 199).all()
    member, gmin = gf.gr2_grids(grid, rng, z)
    assert len(gf.gr2_fit_lines(gmin, int(grid[0] // 200), p)) == 0           # start_index >= bin_num - 1: no lines
    assert gf.ground_removal2(pts).all()


def test_line_fit_against_lstsq():
    rng = np.random.default_rng(3)
    worst = 0.0
    for trial in range(300):
        L = int(rng.integers(2, 200))
        d = np.sort(rng.choice(np.arange(1.0, 100.0, 0.495), L, replace=False)).astype(F)
        z = (rng.uniform(-0.2, 0.2) * d + rng.uniform(-2, 1) + rng.normal(0, 0.05, L)).astype(F)
        m, b = gf.fit_line_f64(d, z)
        (m2, b2), *_ = np.linalg.lstsq(np.stack([d.astype(np.float64), np.ones(L)], axis=1), z.astype(np.float64), rcond=None)
        worst = max(worst, abs(m - m2) / max(abs(m2), 1e-300), abs(b - b2) / max(abs(b2), 1e-300))
    assert worst <= 1e-12, worst


def test_search_step_and_defaults_match_the_library():
    assert gf.gr2_search_step(10.0, 180) == 5
    assert gf.gr2_search_step(0.0, 180) == 0
    d = df.make_filter("GroundRemoval2")
    for name, (arr, slot) in df._PARAMS_EX[df.GROUND_REMOVAL2].items():
        v = d.i[slot] if arr == "i" else d.p[slot]
        assert v == (gf.GR2_DEFAULTS[name] if arr == "i" else F(gf.GR2_DEFAULTS[name])), name
    for t, defaults in ((df.GROUND_REMOVAL, gf.GR_DEFAULTS), (df.RANGE_IMAGE, gf.RI_DEFAULTS)):
        d = df.make_filter(t)
        for name, (arr, slot) in df._PARAMS_EX[t].items():
            assert (d.i[slot] if arr == "i" else d.p[slot]) == (defaults[name] if arr == "i" else F(defaults[name])), name


# ---- RangeImage ----------------------------------------------------------------------------------------------------------
def test_range_image_first_point_of_a_pixel_is_kept():
    pts = rows([[10.0, 0.5, -1.0], [10.0, 0.5, -1.001], [10.0, 0.5, 0.0]])
    assert gf.range_image(pts).tolist() == [True, False, True]


def test_range_image_column_wraps_at_the_last_column():
    pts = rows([[10.0, -1e-4, -1.0], [10.0, 0.0, -1.0]])
    pix = gf.range_image_pixels(pts)
    assert pix[0] == pix[1] and pix[0] % 1800 == 0              # lround gives 1800, wrapped to column 0
    assert gf.range_image(pts).tolist() == [True, False]


def test_range_image_drops_the_axis_and_rows_outside():
    pts = rows([[0.005, 0.0, 0.0], [0.0, 0.009, 1.0], [10.0, 0.0, 10.0], [10.0, 0.0, -5.0], [10.0, 0.0, 0.0]])
    assert gf.range_image(pts).tolist() == [False, False, False, False, True]   # xy < 0.01; above 30 deg; below -15 deg
    assert gf.range_image(pts[3:4], btm_angle=-30.0).tolist() == [True]


# ---- GroundRemoval -------------------------------------------------------------------------------------------------------
def test_ground_removal_truncated_voxel():
    pts = rows([[x, 0.1, 0.05 * k] for k, x in enumerate([-0.5, 0.5] * 5)])   # z spread 0.45 > 0.15: not ground
    assert gf.ground_removal(pts).all()                        # one voxel of 10 (-0.5 and 0.5 share voxel 0)
    vg = of.voxel_grid(pts, 0.8)                               # VoxelGrid's rounding would split them in x
    assert len(np.unique(vg[:, 0])) == 2


def test_ground_removal_small_voxels_vanish():
    pts = rows([[3.1, 3.1 + 0.01 * k, 2.0] for k in range(9)] + [[9.1, 9.1 + 0.01 * k, 2.0] for k in range(10)])
    assert gf.ground_removal(pts).tolist() == [False] * 9 + [True] * 10


def test_ground_removal_z_index_rule():
    def block(z0, spread, x):
        return [[x, 0.3, z0 + spread * k / 9] for k in range(10)]
    pts = rows(block(0.85, 0.1, 1.0) + block(0.0, 0.1, 3.0) + block(-0.7, 0.1, 5.0) + block(-0.9, 0.05, 7.0) + block(-0.3, 0.3, 9.0))
    keep = gf.ground_removal(pts)
    assert keep.reshape(5, 10).all(axis=1).tolist() == [True, False, False, False, True]   # z index 1 kept; spread 0.3 kept


def test_non_finite_rows():
    pts = rows([[np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [5.0, 1.0, 0.0]])
    assert gf.ground_removal(pts).tolist()[:2] == [True, True]
    assert gf.ground_removal2(pts).tolist()[:2] == [True, True]
    assert gf.range_image(pts).tolist() == [False, False, True]


# ---- a synthetic drive ---------------------------------------------------------------------------------------------------
def test_ground_removal2_on_a_synthetic_drive():
    """The commented-out pre-filter of config/lidar_only_kitti.xml on a 120 000-point scan of the seed-5 drive (ground at
    -1.73 m).  The restatement removed 99.9 % of the points within 8 cm of the ground and kept every point 0.5 m or more above
    it; the thresholds leave room below those figures."""
    poses = synth.drive_poses(3, seed=5, speed=8.0, speed_spread=2.0, yaw_rate_max=0.2, segment_s=1.0)
    scene = synth.make_drive_scene(poses, seed=5)
    scan = synth.velodyne_scan(synth.scene_near(scene, poses[1][:3, 3]), poses[1], seed=500, n_points=120_000)
    keep = gf.ground_removal2(of.with_factor(scan), r_min=0.1, start_ground_height=-1.5, long_line_threshold=10, max_slope=0.12,
                              max_error=0.1, max_dist_to_line=0.10, max_start_height=0.6)
    z = scan[:, 2]
    ground, high = np.abs(z + 1.73) < 0.08, z > -1.23
    assert ground.sum() > 10000 and high.sum() > 1000
    assert (~keep[ground]).mean() > 0.95
    assert keep[high].mean() > 0.99


# ---- C descriptor and XML ------------------------------------------------------------------------------------------------
def test_filter_desc_ex_layout(tmp_path):
    src = tmp_path / "layout.c"
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "smhip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(smhip_filter_desc_ex));']
    for name, _ in _capi.FilterDescEx._fields_:
        lines.append(f'  printf("{name} %zu %zu\\n", offsetof(smhip_filter_desc_ex, {name}), sizeof(((smhip_filter_desc_ex*)0)->{name}));')
    lines.append('  printf("ids %d %d %d\\n", SMHIP_FILTER_GROUND_REMOVAL, SMHIP_FILTER_GROUND_REMOVAL2, SMHIP_FILTER_RANGE_IMAGE);')
    src.write_text("\n".join(lines + ["  return 0;", "}"]) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = dict((ln.split()[0], ln.split()[1:]) for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"][0]) == ctypes.sizeof(_capi.FilterDescEx) == 72
    for name, ftype in _capi.FilterDescEx._fields_:
        assert (int(out[name][0]), int(out[name][1])) == (getattr(_capi.FilterDescEx, name).offset, ctypes.sizeof(ftype)), name
    assert out["ids"] == ["6", "7", "8"] and (df.GROUND_REMOVAL, df.GROUND_REMOVAL2, df.RANGE_IMAGE) == (6, 7, 8)


KITTI_XML = """<filters>
  <filter name="Range" ><param type="1" name="min_range"> 5. </param></filter>
  <!-- <filter name="GroundRemoval2" ><param type="1" name="r_min"> 0.1 </param>
       <param type="1" name="start_ground_height"> -1.5 </param></filter> -->
  <filter name="RandomSampler" ><param type="1" name="sampling_rate"> 0.5 </param></filter>
</filters>
<inner_filters>
  <filter name="GroundRemoval2" >
    <param type="1" name="r_min"> 0.1 </param>
    <param type="1" name="start_ground_height"> -0.35 </param>
    <param type="0" name="thread_num"> 4 </param>
  </filter>
  <filter name="RangeImage" ><param type="1" name="btm_angle"> -20. </param><param type="0" name="vertical_line_num"> 60 </param></filter>
</inner_filters>"""


def test_chain_from_xml_opt_in():
    assert [d.type for d in df.chain_from_xml(KITTI_XML)] == [df.RANGE, df.RANDOM_SAMPLER]          # default: unchanged
    chain = df.chain_from_xml(KITTI_XML, ground_filters=True)
    assert [d.type for d in chain] == [df.RANGE, df.RANDOM_SAMPLER, df.GROUND_REMOVAL2, df.RANGE_IMAGE]   # the comment is skipped
    gr2, ri = chain[2], chain[3]
    assert isinstance(gr2, _capi.FilterDescEx) and gr2.p[1] == F(0.1) and gr2.p[2] == F(-0.35) and gr2.i[2] == 4
    assert ri.p[1] == -20.0 and ri.i[0] == 60 and ri.i[1] == 1800
    assert all(df.config_valid(d) for d in chain)
    e = df.widen(chain[0])
    assert e.type == df.RANGE and e.p[0] == 5.0
    with pytest.raises(KeyError):
        df.make_filter("GroundRemoval2", no_such_param=1.0)
