"""Synthetic event windows for tests and bench.py.

Counter-based SplitMix64 so that any language reproduces the same stream:
``u64[i] = mix(seed + (i+1) * 0x9E3779B97F4A7C15)``.  seed = 20200701 + config index
(+ 1000 * window index for further windows of a stream).

Per patch p a ground-truth flow v_p ~ U(-vmax, vmax)^2 px/ms; 90 % of the events
drawn for that patch lie on one of its 1-3 straight edges translating at v_p
(edge point at the event's time, +-1 px jitter), 10 % are uniform noise inside the
patch.  Timestamps are uniform over the 50 ms window and sorted; polarity is a
fair coin; coordinates are clamped into the sensor.
"""
import os

import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
WINDOW_US = 50_000

# BASELINE.json configs: sensor, patch size giving the named patch count with the
# reference's grid rule (feature_detector.cpp:301-346), events per window.
CONFIGS = {
    1: dict(name="C1 240x180 1 patch 10k ev", image=(240, 180), patch=(240, 180), events=10_000),
    2: dict(name="C2 240x180 64 patches 50k ev", image=(240, 180), patch=(30, 22), events=50_000),
    3: dict(name="C3 346x260 256 patches 200k ev", image=(346, 260), patch=(21, 16), events=200_000),
    4: dict(name="C4 1280x720 1024 patches 1M ev", image=(1280, 720), patch=(40, 22), events=1_000_000),
    # the reference's own defaults (DetectorParams): 12x9 patches of 20x20, 15k-event window
    0: dict(name="reference defaults 240x180 108 patches 15k ev", image=(240, 180), patch=(20, 20), events=15_000),
}


def splitmix64(seed, n, start=0):
    """n outputs of the counter-based SplitMix64 stream, starting at counter `start`."""
    with np.errstate(over="ignore"):
        i = np.arange(start + 1, start + n + 1, dtype=np.uint64)
        z = np.uint64(seed) + i * GOLDEN
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def _unit(u64):
    """uint64 -> double in [0,1) with 53 random bits."""
    return (u64 >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def grid_rects(image, patch):
    """Patch rects (x, y, w, h) in row-major grid order, feature_detector.cpp:301-346."""
    iw, ih = image
    pw, ph = patch
    npx, npy = iw // pw, ih // ph
    rects = []
    for y in range(npy):
        for x in range(npx):
            w = pw if x < npx - 1 else iw - x * pw
            h = ph if y < npy - 1 else ih - y * ph
            rects.append((x * pw, y * ph, w, h))
    return npx, npy, np.array(rects, dtype=np.int64)


def make_window(config, window=0, n_events=None, vmax=1.0, t0_us=1_000_000, event_dtype=None):
    """Returns (events structured array sorted by time, ground-truth flows [P][2])."""
    cfg = CONFIGS[config] if not isinstance(config, dict) else config
    idx = config if not isinstance(config, dict) else cfg.get("index", 9)
    seed = 20200701 + idx + 1000 * window
    iw, ih = cfg["image"]
    npx, npy, rects = grid_rects(cfg["image"], cfg["patch"])
    P = npx * npy
    N = int(n_events if n_events is not None else cfg["events"])

    # per-patch draws: 2 (flow) + 1 (edge count) + 3 edges * 4
    pp = _unit(splitmix64(seed, P * 15)).reshape(P, 15)
    flow = (pp[:, 0:2] * 2.0 - 1.0) * vmax
    n_edges = 1 + (pp[:, 2] * 3.0).astype(np.int64)
    rx, ry, rw, rh = [rects[:, k].astype(np.float64) for k in range(4)]
    ex = rx[:, None] + pp[:, 3:6] * rw[:, None]
    ey = ry[:, None] + pp[:, 6:9] * rh[:, None]
    eth = pp[:, 9:12] * np.pi
    elen = (0.25 + 0.25 * pp[:, 12:15]) * np.minimum(rw, rh)[:, None]

    # per-event draws: 8 each
    ee = _unit(splitmix64(seed, N * 8, start=P * 15)).reshape(N, 8)
    t = np.sort((ee[:, 0] * WINDOW_US).astype(np.int64), kind="stable")
    pid = np.minimum((ee[:, 1] * P).astype(np.int64), P - 1)
    noise = ee[:, 2] < 0.1
    eidx = np.minimum((ee[:, 3] * n_edges[pid]).astype(np.int64), n_edges[pid] - 1)
    s = ee[:, 4] * 2.0 - 1.0
    jx = np.floor(ee[:, 5] * 3.0) - 1.0
    jy = np.floor(ee[:, 6] * 3.0) - 1.0
    pol = np.where(ee[:, 7] < 0.5, -1, 1)

    dt_ms = (t.astype(np.float64) - WINDOW_US / 2.0) * 1e-3
    th = eth[pid, eidx]
    px = ex[pid, eidx] + s * elen[pid, eidx] * np.cos(th) + flow[pid, 0] * dt_ms + jx
    py = ey[pid, eidx] + s * elen[pid, eidx] * np.sin(th) + flow[pid, 1] * dt_ms + jy
    nx = rx[pid] + ee[:, 4] * rw[pid]
    ny = ry[pid] + ee[:, 5] * rh[pid]
    x = np.where(noise, nx, px)
    y = np.where(noise, ny, py)
    xi = np.clip(np.floor(x), 0, iw - 1).astype(np.int32)
    yi = np.clip(np.floor(y), 0, ih - 1).astype(np.int32)

    if event_dtype is None:
        event_dtype = np.dtype(
            [("x", "<i4"), ("y", "<i4"), ("sign", "<i4"), ("reserved", "<i4"), ("t_us", "<i8")])
    ev = np.zeros(N, dtype=event_dtype)
    ev["x"] = xi
    ev["y"] = yi
    ev["sign"] = pol
    ev["t_us"] = t + t0_us + window * WINDOW_US
    return ev, flow


def make_stream(config, n_windows, **kw):
    """n_windows consecutive windows: (events, offsets [n+1], flows [n][P][2])."""
    evs, flows = [], []
    for w in range(n_windows):
        e, f = make_window(config, window=w, **kw)
        evs.append(e)
        flows.append(f)
    offsets = np.zeros(n_windows + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(e) for e in evs])
    return np.concatenate(evs), offsets, np.stack(flows)


def write_events_txt(path, ev):
    """DAVIS events.txt format (davis240c_reader.cpp:60-92): '<sec> <x> <y> <0|1>'."""
    with open(path, "w") as fp:
        for e in ev:
            fp.write("%.9f %d %d %d\n" % (int(e["t_us"]) * 1e-6, e["x"], e["y"], 1 if e["sign"] > 0 else 0))


# ---- a DAVIS recording directory: frames, events, ground truth, calibration --------------------------------------
def png8_bytes(img, filters=0, level=6, strategy=None, idat_split=None):
    """An 8-bit greyscale, non-interlaced PNG of `img` (uint8 [h][w]) written with Python's zlib.  `filters`: one row
    filter type 0-4 for every row, or a sequence of one per row; `level` 0-9 and `strategy` (zlib.Z_FILTERED,
    Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED; None = Z_DEFAULT_STRATEGY) choose the deflate blocks; `idat_split` cuts the
    stream into IDAT chunks of that many bytes (None: one chunk)."""
    import struct
    import zlib

    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape
    kinds = [int(filters)] * h if np.isscalar(filters) else [int(f) for f in filters]
    raw = bytearray()
    prev = np.zeros(w, dtype=np.int32)
    for y in range(h):
        cur = img[y].astype(np.int32)
        left = np.concatenate(([0], cur[:-1]))
        upleft = np.concatenate(([0], prev[:-1]))
        f = kinds[y]
        if f == 0:
            pred = np.zeros(w, dtype=np.int32)
        elif f == 1:
            pred = left
        elif f == 2:
            pred = prev
        elif f == 3:
            pred = (left + prev) >> 1
        elif f == 4:
            p = left + prev - upleft
            pa, pb, pc = np.abs(p - left), np.abs(p - prev), np.abs(p - upleft)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, upleft))
        else:
            raise ValueError("row filter %d" % f)
        raw.append(f)
        raw += ((cur - pred) & 255).astype(np.uint8).tobytes()
        prev = cur
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, zlib.Z_DEFAULT_STRATEGY if strategy is None else strategy)
    stream = co.compress(bytes(raw)) + co.flush()

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)

    step = len(stream) if not idat_split else int(idat_split)
    idats = b"".join(chunk(b"IDAT", stream[i:i + step]) for i in range(0, max(len(stream), 1), max(step, 1)))
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) + idats +
            chunk(b"IEND", b""))


def _smooth_texture(rng, h, w, sigma=2.0):
    big = rng.uniform(0.0, 1.0, size=(h, w))
    r = int(3 * sigma)
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    big = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), 1, big)
    big = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), 0, big)
    big = (big - big.mean()) / (big.std() + 1e-12)
    return np.clip(128.0 + 45.0 * big, 8.0, 247.0)


def _bilinear(tex, x, y):
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    ax, ay = x - x0, y - y0
    return ((1 - ay) * ((1 - ax) * tex[y0, x0] + ax * tex[y0, x0 + 1]) +
            ay * ((1 - ax) * tex[y0 + 1, x0] + ax * tex[y0 + 1, x0 + 1]))


def _undistorted_grid(px, py, focal, cx, cy, k1, k2, p1, p2, iterations=60):
    """The undistorted pixel position of every distorted pixel (px, py): the fixed point of the radial-tangential
    model, iterated until it no longer moves (60 steps are far beyond convergence for a lens that is invertible over
    the sensor)."""
    xd = (px - cx) / focal
    yd = (py - cy) / focal
    x, y = xd.copy(), yd.copy()
    for _ in range(iterations):
        r2 = x * x + y * y
        radial = 1.0 + k1 * r2 + k2 * r2 * r2
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = 2.0 * p2 * x * y + p1 * (r2 + 2.0 * y * y)
        x = (xd - dx) / radial
        y = (yd - dy) / radial
    return focal * x + cx, focal * y + cy


def make_recording(path, seed=0, size=(240, 180), duration_s=0.8, fps=24.0, velocity=(40.0, -25.0), threshold=0.25,
                   step_us=1000, focal=200.0, distortion=None, angular_velocity=None):
    """Writes a DAVIS240C recording directory at `path`: events.txt, images.txt + images/frame_<i>.png,
    groundtruth.txt and calib.txt.

    The scene is a seeded smooth random texture translating across the sensor at `velocity` (px/s): the frame at time
    t is the texture sampled (bilinear) at x - vx t, y - vy t.  Events are ESIM-style: every `step_us` the log
    intensity of each pixel is compared with its last reference level, and every crossing of `threshold` emits an
    event (+1 up, -1 down) at a time spread evenly inside the step; the reference moves by the crossings.  Frames
    (8-bit grey PNG, written with Python's zlib) every 1/fps s from t = 1/fps.  Ground truth: the camera translating
    parallel to a plane at depth 1, t = (-vx, -vy, 0) * t / focal, identity rotation; calib.txt: focal, focal, the
    sensor centre, no distortion.  Returns dict(events=n, frames=n, velocity=(vx, vy)).

    distortion=(k1, k2, p1, p2): the sensor sits behind a lens with these radial-tangential coefficients (the camera
    model of include/ebo.h with fx = fy = focal and the sensor centre).  A point of the ideal pinhole image appears at
    `project` of its position: sensor pixel (x, y) shows the scene at its undistorted position, found by iterating the
    model's fixed point to convergence.  calib.txt then carries the coefficients (k3 = 0).  The default (None) writes
    exactly what this function wrote before the keyword existed.

    angular_velocity=(wx, wy, wz) in rad/s, camera frame: the scene rotates about the camera centre instead of
    translating (`velocity` is ignored).  A static point moves by dX/dt = -omega x X in the camera frame, so the pixel
    whose ray is X at time t shows the texture where project(R(omega t) X) falls, R the exact (Rodrigues) rotation.
    groundtruth.txt then carries the rotation: zero translation and the quaternion (x y z w) of exp([omega]x t), camera
    to world.  The default (None) writes exactly what this function wrote before the keyword existed."""
    w, h = size
    rng = np.random.default_rng(20240601 + seed)
    vx, vy = velocity
    margin = int(np.ceil(max(abs(vx), abs(vy)) * duration_s)) + 4
    gx, gy = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    if distortion is not None:
        gx, gy = _undistorted_grid(gx, gy, focal, w / 2.0, h / 2.0, *[float(v) for v in distortion])
        margin += int(np.ceil(max(-gx.min(), gx.max() - (w - 1), -gy.min(), gy.max() - (h - 1), 0.0)))
    if angular_velocity is not None:
        om = np.array([float(v) for v in angular_velocity])
        rays = np.stack([(gx - w / 2.0) / focal, (gy - h / 2.0) / focal, np.ones_like(gx)], axis=-1)

        def source(t_us):
            """Where in the pinhole image of t = 0 every pixel of time t looks."""
            rv = om * (t_us * 1e-6)
            th = float(np.linalg.norm(rv))
            R = np.eye(3)
            if th > 0.0:
                kx, ky, kz = rv / th
                K = np.array([[0.0, -kz, ky], [kz, 0.0, -kx], [-ky, kx, 0.0]])
                R = np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)
            X = rays @ R.T
            return focal * X[..., 0] / X[..., 2] + w / 2.0, focal * X[..., 1] / X[..., 2] + h / 2.0

        margin = 4
        for t_us in np.linspace(0.0, duration_s * 1e6, 17):
            sx, sy = source(t_us)
            margin = max(margin, 4 + int(np.ceil(max(-sx.min(), sx.max() - (w - 1), -sy.min(), sy.max() - (h - 1), 0.0))))
    tex = _smooth_texture(rng, h + 2 * margin, w + 2 * margin)

    def render(t_us):
        if angular_velocity is not None:
            sx, sy = source(t_us)
            return _bilinear(tex, sx + margin, sy + margin)
        t = t_us * 1e-6
        return _bilinear(tex, gx + margin - vx * t, gy + margin - vy * t)

    os.makedirs(os.path.join(path, "images"), exist_ok=True)
    # events
    ref = np.log(render(0))
    chunks = []
    n_steps = int(duration_s * 1e6) // step_us
    for k in range(1, n_steps + 1):
        t1 = k * step_us
        L = np.log(render(t1))
        d = L - ref
        n = np.floor(np.abs(d) / threshold).astype(np.int64)
        ys, xs = np.nonzero(n)
        if len(ys):
            cnt = n[ys, xs]
            sgn = np.sign(d[ys, xs]).astype(np.int64)
            ref[ys, xs] += sgn * cnt * threshold
            rep = np.repeat(np.arange(len(ys)), cnt)
            j = np.arange(len(rep)) - np.repeat(np.cumsum(cnt) - cnt, cnt)  # 0..cnt-1 inside each pixel
            t = (t1 - step_us) + ((j + 1) * step_us) // (cnt[rep] + 1)
            chunks.append(np.stack([t, xs[rep], ys[rep], (sgn[rep] > 0).astype(np.int64)], axis=1))
    ev = np.concatenate(chunks) if chunks else np.zeros((0, 4), dtype=np.int64)
    ev = ev[np.argsort(ev[:, 0], kind="stable")]
    with open(os.path.join(path, "events.txt"), "w") as f:
        f.write("".join("%d.%06d000 %d %d %d\n" % (t // 1000000, t % 1000000, x, y, p) for t, x, y, p in ev))
    # frames
    lines = []
    period_us = int(round(1e6 / fps))
    t = period_us
    i = 0
    while t <= n_steps * step_us:
        img = np.clip(np.rint(render(t)), 0, 255).astype(np.uint8)
        name = "images/frame_%08d.png" % i
        with open(os.path.join(path, name), "wb") as f:
            f.write(png8_bytes(img, filters=4, level=6))
        lines.append("%d.%06d000 %s\n" % (t // 1000000, t % 1000000, name))
        t += period_us
        i += 1
    with open(os.path.join(path, "images.txt"), "w") as f:
        f.write("".join(lines))
    with open(os.path.join(path, "groundtruth.txt"), "w") as f:
        for k in range(0, n_steps + 1, 10):
            ts = k * step_us
            if angular_velocity is not None:
                rv = om * (ts * 1e-6)
                th = float(np.linalg.norm(rv))
                q = np.append(rv / th * np.sin(th / 2.0), np.cos(th / 2.0)) if th > 0.0 else np.array([0.0, 0.0, 0.0, 1.0])
                f.write("%d.%06d000 0.0 0.0 0.0 %.9f %.9f %.9f %.9f\n" % ((ts // 1000000, ts % 1000000) + tuple(q)))
                continue
            f.write("%d.%06d000 %.9f %.9f 0.0 0.0 0.0 0.0 1.0\n" % (ts // 1000000, ts % 1000000,
                                                                   -vx * ts * 1e-6 / focal, -vy * ts * 1e-6 / focal))
    with open(os.path.join(path, "calib.txt"), "w") as f:
        if distortion is None:
            f.write("%g %g %g %g 0 0 0 0 0\n" % (focal, focal, w / 2.0, h / 2.0))
        else:  # calib.txt's order: fx fy cx cy k1 k2 p1 p2 k3
            f.write("%g %g %g %g %s 0\n" % (focal, focal, w / 2.0, h / 2.0, " ".join(repr(float(v)) for v in distortion)))
    if angular_velocity is not None:
        return dict(events=len(ev), frames=i, velocity=(vx, vy), angular_velocity=tuple(float(v) for v in om))
    return dict(events=len(ev), frames=i, velocity=(vx, vy))
