"""Times one frame of the device image front end (FeatureDetector::newImage's goodFeaturesToTrack, log image +
Sobel and calcOpticalFlowPyrLK): ebo_image_gradients + ebo_good_features (the reference's mask and maxCorners_,
patchExtent 12) + ebo_lk_add_image + ebo_lk_track of the detected points, with device events around the frame
after a warm-up.  240x180 is the DAVIS fixture frame pair; 346x260 and 640x480 are synthetic smoothed textures
moved by (1.5, -0.75) px.
usage: python time_front_end.py [REPS]"""
import importlib
import os
import sys

import numpy as np

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


def one_frame(c, a, b, mask, max_corners):
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
            c.lk_add_image(a)
            for _ in range(3):  # warm-up: code objects, workspaces
                one_frame(c, a, b, mask, max_corners)
            times = []
            for _ in range(reps):
                c.lk_add_image(a)
                c.timer_begin()
                n, ok = one_frame(c, a, b, mask, max_corners)
                times.append(c.timer_end())
        times = np.array(times)
        print(f"{w}x{h}: maxCorners {max_corners}, corners {n}, tracked {ok}: per frame median {np.median(times):.3f} ms "
              f"(min {times.min():.3f}, max {times.max():.3f}, {reps} frames; device events around the four calls, "
              f"host copies and synchronisations included)", flush=True)


if __name__ == "__main__":
    main()
