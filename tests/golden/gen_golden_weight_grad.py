"""Generate tests/golden/weight_grad.npz by RUNNING THE REFERENCE with the per-event `weight` on the autograd tape.

Run in the build container only (needs the reference checkout, see ref_import.py):
    python tests/golden/gen_golden_weight_grad.py
Data only.  The reference is imported in place through ref_import.py (stubs + 3 shims; shim (1), the 3-tap blur, reaches the sigma 1
cases).  Per case: Warp.warp_event -> EventImageConverter.create_image_from_events_tensor(weight=w, sigma) per image the cost reads
(the steps of PatchContrastMaximization.get_arg_for_cost, src/solver/patch_contrast_base.py:289-352, with the weight handed to the
vote, src/event_image_converter.py:126-158, 316-372) -> costs.functions[cost].calculate -> loss.backward() -> w.grad.

Cases: 24 x 32 sensor, 500 events, the three motion models (voxel T = 2) x {image_variance sigma 0, gradient_magnitude sigma 1,
normalized_image_variance sigma 0, multi_focal_normalized_gradient_magnitude sigma 1}."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

src = ref_import.import_reference()
from src import costs, event_image_converter, warp  # noqa: E402

SEED = 47
H, W, N, T = 24, 32, 500, 2
CASES = [("image_variance", 0), ("gradient_magnitude", 1), ("normalized_image_variance", 0), ("multi_focal_normalized_gradient_magnitude", 1)]
IMAGE_DIRECTION = {"iwe": "first", "forward_iwe": "last", "middle_iwe": "middle"}


def main():
    rng = np.random.default_rng(SEED)
    ev = np.stack([rng.uniform(0, H - 1, N), rng.uniform(0, W - 1, N), np.sort(rng.uniform(0.0, 0.05, N)), rng.integers(0, 2, N).astype(np.float64)], axis=1)
    wgt = rng.uniform(0.2, 3.0, N)
    wgt[::9] = 0.0
    motions = {"2dof": ("2d-translation", np.array([37.0, -52.0])), "dense": ("dense-flow", rng.normal(0, 40, (2, H, W))),
               "voxel": ("dense-flow-voxel", rng.normal(0, 40, (T, 2, H, W)))}
    out = dict(events=ev, weights=wgt, image_size=np.array([H, W]), shims=np.array(ref_import.SHIMS))
    warper = warp.Warp((H, W), calculate_feature=True, normalize_t=True)
    imager = event_image_converter.EventImageConverter((H, W))
    te = torch.from_numpy(ev)
    for mname, (model, motion) in motions.items():
        out["motion_" + mname] = motion
        tm = torch.from_numpy(motion)
        for cost, sigma in CASES:
            cf = costs.functions[cost](direction="minimize", store_history=False, image_size=(H, W), percentile=1.0, precision="64", cuda_available=False)
            w = torch.from_numpy(wgt.copy()).requires_grad_()
            arg = {"omit_boundary": True, "clip": True}
            if "orig_iwe" in cf.required_keys:
                arg["orig_iwe"] = imager.create_image_from_events_tensor(te, "bilinear_vote", weight=w, sigma=sigma)
            for key, direction in IMAGE_DIRECTION.items():
                if key in cf.required_keys or (key == "iwe" and "backward_iwe" in cf.required_keys):
                    warped, _ = warper.warp_event(te, tm, model, direction=direction)
                    arg[key] = imager.create_image_from_events_tensor(warped, "bilinear_vote", weight=w, sigma=sigma)
                    if key == "iwe":
                        arg["backward_iwe"] = arg[key]
            loss = cf.calculate(arg)
            loss.backward()
            tag = f"{mname}__{cost}__s{sigma}"
            out[tag + "__loss"] = np.array(loss.item())
            out[tag + "__grad_w"] = w.grad.numpy().copy()
    path = os.path.join(HERE, "weight_grad.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(CASES) * len(motions), "cases")


if __name__ == "__main__":
    main()
