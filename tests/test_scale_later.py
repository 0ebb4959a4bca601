"""Host-side checks of `solver.scale_later` (src/solver/base.py:219-224): the solver class takes the key, the descriptor that
carries it to the library has the library's layout, and the fixture of the GPU tests is data only."""
import ctypes
import os

import numpy as np

import event_based_optical_flow_amd as E
from event_based_optical_flow_amd import _lib

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solver_scale_later.npz")
OPT_CFG = {"n_iter": 40, "method": "Newton-CG", "max_iter": 25,
           "parameters": {"trans_x": {"min": -150, "max": 150}, "trans_y": {"min": -150, "max": 150}}}


def _config(**extra):
    cfg = {"method": "pyramidal_patch_contrast_maximization", "time_aware": True, "time_bin": 10, "flow_interpolation": "burgers",
           "t0_flow_location": "middle",
           "patch": {"initialize": "random", "scale": 4, "crop_height": 64, "crop_width": 80, "filter_type": "bilinear"},
           "motion_model": "2d-translation", "warp_direction": "first", "parameters": ["trans_x", "trans_y"], "cost": "hybrid",
           "outer_padding": 0, "cost_with_weight": {"multi_focal_normalized_gradient_magnitude": 1.0, "total_variation": 0.01},
           "iwe": {"method": "bilinear_vote", "blur_sigma": 1}}
    cfg.update(extra)
    return cfg


def test_solver_class_takes_scale_later():
    make = E.solver.collections["pyramidal_patch_contrast_maximization"]
    assert make((68, 90), {}, _config(scale_later=True), OPT_CFG, {}, None).scale_later is True
    assert make((68, 90), {}, _config(scale_later=False), OPT_CFG, {}, None).scale_later is False
    assert make((68, 90), {}, _config(), OPT_CFG, {}, None).scale_later is False
    # without time_aware the reference never reads the key
    assert make((68, 90), {}, _config(time_aware=False, scale_later=True), OPT_CFG, {}, None).scale_later is False


def test_descriptor_layout_and_abi_version():
    lib = _lib.load()
    assert ctypes.sizeof(_lib.CmaxPatchObjective) == lib.cmax_sizeof_patch_objective()
    assert lib.cmax_abi_version() == _lib.ABI_VERSION
    d = _lib.CmaxPatchObjective()
    d.scale_later = 1
    assert d.scale_later == 1 and _lib.CmaxPatchObjective.scale_later.offset < _lib.CmaxPatchObjective.t_scale.offset
    for name in ("cmax_field_max", "cmax_field_max_adj"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES


def test_fixture_is_data_only():
    with np.load(GOLD, allow_pickle=False) as g:  # allow_pickle=False: no object arrays, hence no code
        keys = list(g.keys())
        for k in keys:
            assert g[k].dtype.kind in "fiuUS", (k, g[k].dtype)
        cases = [str(c) for c in g["cases"]]
        assert len(cases) == 7
        for c in cases:
            for field in ("x", "loss", "grad", "v", "vhp", "scale", "n_ties", "voxel_tensor", "voxel_numpy", "loss_off"):
                assert f"{c}__{field}" in keys
            # the generator's separation: a build that ignores the flag cannot pass at the tests' tolerance
            assert abs(float(g[c + "__loss"]) - float(g[c + "__loss_off"])) > float(g["separation"]) * abs(float(g[c + "__loss"]))
        assert int(g["interior_s3__n_ties"]) == 1 and int(g["plateau_s3__n_ties"]) > 1 and float(g["negative_s3__scale"]) < 0
