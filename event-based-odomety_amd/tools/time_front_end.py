"""Times one frame of the device image front end (FeatureDetector::newImage's goodFeaturesToTrack, log image +
Sobel and calcOpticalFlowPyrLK): ebo_image_gradients + ebo_good_features (the reference's mask and maxCorners_,
patchExtent 12) + ebo_lk_add_image + ebo_lk_track of the detected points, with device events around the frame
after a warm-up.  240x180 is the DAVIS fixture frame pair; 346x260 and 640x480 are synthetic smoothed textures
moved by (1.5, -0.75) px.  Each size is timed twice, without and with the frame remap of ebo_rectify_image in front
of the four calls (the DAVIS240C lens scaled to the sensor, the fitted rectified camera), and the remap kernel alone
(ebo_rectify_image_device on resident frames) by stream events.
usage: python time_front_end.py [REPS]"""
import importlib
import os
import sys

import numpy as np
import torch  # noqa: F401  (before the library: see tests/conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ebo = importlib.import_module("event-based-odomety_amd")
F = importlib.import_module("frontend_ref")

PATCH_EXTENT = 12


def frame_pair(w, h):
    if (w, h) == (240, 180):
        fr = F.frames()
        return fr[0], fr[1]
    return F.shifted(F.textured(h, w, seed=w, sigma=2.0), h, w, 1.5, -0.75)


LENS = (-0.368436311798, 0.150947243557, 0.0, -0.000296130534385, -0.000759431726241)


def lens(w, h):
    return (199.092366542 * w / 240.0, 198.82882047 * h / 180.0, 132.192071378 * w / 240.0, 110.712660011 * h / 180.0) + LENS


def one_frame(c, a, b, mask, max_corners, remap=False):
    if remap:
        b = c.rectify_image(b)
    c.image_gradients(b)
    pts = c.good_features(a, mask=mask, max_corners=max_corners)
    c.lk_add_image(b)
    _, st, _ = c.lk_track(pts)
    return len(pts), int(st.sum())


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    for w, h in ((240, 180), (346, 260), (640, 480)):
        a, b = frame_pair(w, h)
        mask = F.reference_mask(w, h, PATCH_EXTENT)
        max_corners = F.reference_max_corners(w, h, PATCH_EXTENT)
        with ebo.Context(image_w=w, image_h=h) as c:
            c.set_rectification_camera(lens(w, h), c.fit_rectified_camera(lens(w, h)))
            for remap in (False, True):
                first = c.rectify_image(a) if remap else a
                c.lk_add_image(first)
                for _ in range(3):  # warm-up: code objects, workspaces
                    one_frame(c, first, b, mask, max_corners, remap)
                times = []
                for _ in range(reps):
                    c.lk_add_image(first)
                    c.timer_begin()
                    n, ok = one_frame(c, first, b, mask, max_corners, remap)
                    times.append(c.timer_end())
                times = np.array(times)
                print(f"{w}x{h}{' + remap' if remap else ''}: maxCorners {max_corners}, corners {n}, tracked {ok}: per frame "
                      f"median {np.median(times):.3f} ms (min {times.min():.3f}, max {times.max():.3f}, {reps} frames; device "
                      f"events around the {'five' if remap else 'four'} calls, host copies and synchronisations included)",
                      flush=True)
            d_in = torch.from_numpy(b).to("cuda")
            d_out = torch.zeros_like(d_in)
            torch.cuda.synchronize()
            kernel = []
            for _ in range(reps + 3):
                c.timer_begin()
                c.rectify_image_device(d_in.data_ptr(), d_out.data_ptr())
                kernel.append(c.timer_end())
            kernel = np.array(kernel[3:])
            print(f"{w}x{h}: k_rectify_image alone median {np.median(kernel) * 1e3:.1f} us (min {kernel.min() * 1e3:.1f}, "
                  f"max {kernel.max() * 1e3:.1f}; stream events around one launch)", flush=True)


if __name__ == "__main__":
    main()
