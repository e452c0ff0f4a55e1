"""GPU: the integer count images where their per-path machinery decides -- at rounding ties of the float pre-test, at the
limits of the packed 16-bit counters, on the seams of tiles and bands, and in every store form.  The cases come from
tests/count_cases.py (tests/test_count_cases_cpu.py checks on the CPU that they have the teeth claimed here, and
tests/cpp/count_plan_test.cpp pins the kernel every forced shape runs); every assertion is np.array_equal against the
oracle, and every forced path is also compared with the global-atomics path (impl 0)."""
import numpy as np
import pytest

import count_cases as cc

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _prm(orc, c):
    return orc.default_params(image_w=c["w"], image_h=c["h"], patch_w=c["pw"], patch_h=c["ph"], scale=c["scale"], loss=1)


def oracle_images(orc, c):
    """The oracle's images of a case, computed once and shared by the tests that need them (read-only)."""
    if c["name"] not in _ORACLE:
        out = []
        for k in range(len(c["offsets"]) - 1):
            ev = cc.window_events(c, k)
            if c["flows"] is not None:
                out.append(orc.final_count_image(ev, _prm(orc, c), c["flows"][k]))
            elif c["field"] is not None:
                out.append(orc.compensate_events_field(ev, c["w"], c["h"], c["field"][k], scale=c["scale"]))
            else:
                out.append(orc.integrate_events(ev, c["w"], c["h"]))
        img = np.stack(out)
        img.setflags(write=False)
        _ORACLE[c["name"]] = img
    return _ORACLE[c["name"]]


def _context(ebo, c, **kw):
    return ebo.Context(image_w=c["w"], image_h=c["h"], patch_w=c["pw"], patch_h=c["ph"], scale=c["scale"],
                       loss=ebo.LOSS_VARIANCE, tv_weight=0.0, max_windows=len(c["offsets"]) - 1, max_events=len(c["ev"]), **kw)


def _count(ebo, ctx, c):
    if c["flows"] is not None:
        return ctx.count_image(ebo.COUNT_WARPED, c["flows"])
    if c["field"] is not None:
        return ctx.count_image(ebo.COUNT_FIELD, c["field"])
    return ctx.count_image(ebo.COUNT_INTEGRATED)


_KNOBS = ("EBO_COUNT_IMPL", "EBO_COUNT_LDS_KB", "EBO_COUNT_TILE_W", "EBO_COUNT_TILE_H", "EBO_COUNT_BLOCK")


def _force(monkeypatch, impl, lds_kb=0, tile=None, block=0):
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    if impl is not None:
        monkeypatch.setenv("EBO_COUNT_IMPL", str(impl))
    if lds_kb:
        monkeypatch.setenv("EBO_COUNT_LDS_KB", str(lds_kb))
    if tile:
        monkeypatch.setenv("EBO_COUNT_TILE_W", str(tile[0]))
        monkeypatch.setenv("EBO_COUNT_TILE_H", str(tile[1]))
    if block:
        monkeypatch.setenv("EBO_COUNT_BLOCK", str(block))


def _where(got, want):
    """The first pixels that differ, for the failure message."""
    at = np.argwhere(got != want)[:6]
    return [(tuple(int(v) for v in a), float(got[tuple(a)]), float(want[tuple(a)])) for a in at]


def _check_forced(ebo_ab, orc, monkeypatch, c, impl, **knobs):
    """Case c on the forced path and on impl 0 in one context: both equal the oracle's images."""
    want = oracle_images(orc, c)
    with _context(ebo_ab, c) as ctx:
        ctx.set_windows(c["ev"], c["offsets"])
        _force(monkeypatch, impl, **knobs)
        got = _count(ebo_ab, ctx, c)
        _force(monkeypatch, 0)
        plain = _count(ebo_ab, ctx, c)
    assert np.array_equal(plain, want), (c["name"], "impl 0", _where(plain, want))
    assert np.array_equal(got, want), (c["name"], impl, knobs, _where(got, want))
    assert np.array_equal(got, plain)


# the seams of each path: (tile_w, tile_h, n_windows) of count_cases.seams and the knobs that give the path that pitch
# (tests/cpp/count_plan_test.cpp, "seams ...")
_SEAMS = {0: ((0, 25, 0), {}), 1: ((0, 25, 0), dict(lds_kb=12)), 3: ((0, 25, 0), dict(lds_kb=12)),
          4: ((0, 23, 0), dict(lds_kb=12)), 5: ((30, 23, 8), {})}


@pytest.mark.parametrize("impl", [0, 1, 3, 4, 5])
@pytest.mark.parametrize("sensor", ["small", "wide", "tall"])
def test_warped_ties_on_every_path(ebo_ab, orc, monkeypatch, sensor, impl):
    """k + 0.5 + delta from one ulp to 1e-4 on both sides, both axes, displacements from 0.5 to 16000 pixels, times up to
    2^24 us, positions from -0.5 to extent - 0.5: count_target's float pre-test (impl 1, 3, 4; the stray kernel) and
    count_hit_uniform's per-unit one (impl 5) must send every event they cannot vouch for to the f64 expression."""
    _check_forced(ebo_ab, orc, monkeypatch, cc.ties_warped(sensor), impl)


@pytest.mark.parametrize("impl", [0, 1, 3, 4, 5])
def test_warped_seams_on_every_path(ebo_ab, orc, monkeypatch, impl):
    """Events at their unit's largest |dt| that land on the first and last row / column of tiles and bands one and two
    pitches away, and on the seam's tie: a unit selected by reach that falls one pixel short loses them."""
    pitch, knobs = _SEAMS[impl]
    _check_forced(ebo_ab, orc, monkeypatch, cc.seams(*pitch), impl, **knobs)


@pytest.mark.parametrize("tile,block", [((8, 8), 0), ((8, 6), 64)])
def test_warped_ties_on_small_tiles(ebo_ab, orc, monkeypatch, tile, block):
    """k_count_tiles with tiles of 8 x 8 pixels and of one patch (8 x 6), the latter with one wave per workgroup."""
    _check_forced(ebo_ab, orc, monkeypatch, cc.ties_warped("small"), 5, tile=tile, block=block)


@pytest.mark.parametrize("tile", [(8, 8), (30, 22)])
def test_warped_seams_on_small_tiles(ebo_ab, orc, monkeypatch, tile):
    _check_forced(ebo_ab, orc, monkeypatch, cc.seams(tile[0], tile[1], 0), 5, tile=tile)


@pytest.mark.parametrize("impl", [0, 1, 3])
@pytest.mark.parametrize("sensor", ["small", "wide", "tall"])
def test_field_ties_on_every_path(ebo_ab, orc, monkeypatch, sensor, impl):
    _check_forced(ebo_ab, orc, monkeypatch, cc.ties_field(sensor), impl)


@pytest.mark.parametrize("case", ["c2 warped: tiles", "fine warped: unit waves", "c2x64 field: whole-window LDS"])
def test_ties_on_the_plan_the_shipped_library_makes(ebo, orc, case):
    """The same ladders in batches whose plan is k_count_tiles, k_count_units and k_count_window_lds without any switch
    (tests/cpp/count_plan_test.cpp, "ties C2x24", "ties fine x32", "ties C2x64 field")."""
    sensor = case.split()[0]
    c = cc.ties_field(sensor) if "field" in case else cc.ties_warped(sensor)
    want = oracle_images(orc, c)
    with _context(ebo, c) as ctx:
        ctx.set_windows(c["ev"], c["offsets"])
        got = _count(ebo, ctx, c)
    assert np.array_equal(got, want), (case, _where(got, want))


def _shards(ebo, c, n_windows, world):
    """The first n_windows windows of a warped case cut into `world` row shards of the patch grid, as
    tests/test_gpu_shard.py cuts them."""
    from test_gpu_shard import _shard_events
    npx, npy = cc.grid(c["w"], c["h"], c["pw"], c["ph"])
    evs = [cc.window_events(c, k) for k in range(n_windows)]
    S = dict(evs=evs, npx=npx, npy=npy, pw=c["pw"], ph=c["ph"])
    xr, yr = cc._ranges(c["w"], c["pw"]), cc._ranges(c["h"], c["ph"])
    rects = np.array([(xr[p % npx][0], yr[p // npx][0], xr[p % npx][1] - xr[p % npx][0] + 1,
                       yr[p // npx][1] - yr[p // npx][0] + 1) for p in range(npx * npy)])
    t_ref = [cc.ref_time(e["t_us"][0], e["t_us"][-1]) for e in evs]
    out = []
    for r in range(world):
        b, e = ebo.shard_range(npy, r, world)
        my, sev, soffs = _shard_events(S, b, e, n_windows)
        out.append(dict(rows=(yr[b][0], yr[e - 1][1] + 1), my=my, ev=sev, offs=soffs, rects=np.tile(rects[my], (n_windows, 1))))
    return out, t_ref, evs


def _shard_kw(ebo, c, n_windows, n_events):
    return dict(image_w=c["w"], image_h=c["h"], patch_w=c["pw"], patch_h=c["ph"], scale=c["scale"], loss=ebo.LOSS_VARIANCE,
                tv_weight=0.0, max_events=n_events, max_windows=n_windows)


def test_ties_through_the_shard_images(ebo, orc):
    """k_count_shard (count_target per event, f64 atomics): the partial images of three row shards sum to the oracle's."""
    c = cc.ties_warped("c2")
    n_windows = 6
    want = oracle_images(orc, c)[:n_windows]
    shards, t_ref, evs = _shards(ebo, c, n_windows, 3)
    total = np.zeros_like(want)
    for sh in shards:
        with ebo.Context(**_shard_kw(ebo, c, n_windows, len(sh["ev"]))) as ctx:
            ctx.set_patches(sh["ev"], sh["offs"], sh["rects"])
            part = ctx.count_image_shard(n_windows, t_ref, c["flows"][:n_windows])
        assert np.array_equal(part, np.round(part)) and part.min() >= 0
        total += part
    assert np.array_equal(total, want), _where(total, want)


@pytest.mark.parametrize("halo", [70, 16])
def test_ties_through_the_band_images(ebo, orc, halo):
    """k_count_band on two row shards: with a halo beyond every unit's reach nothing escapes and own rows + received
    halos are the oracle's image; with 16 rows the units 30 to 60 pixels of y displacement near the border raise the flag.
    `escaped` is compared with the rule restated from the geometry: a unit's event rows grown by
    max|dt| x |scale| x |flow_y| + 1 must stay inside the band (or the band must end at the image's border)."""
    import torch
    c = cc.ties_warped("c2")
    n_windows, world = 6, 2
    iw, ih = c["w"], c["h"]
    want = oracle_images(orc, c)[:n_windows]
    shards, t_ref, evs = _shards(ebo, c, n_windows, world)
    bounds = [sh["rows"][0] for sh in shards] + [ih]
    flows = np.ascontiguousarray(c["flows"][:n_windows])
    d_flows = torch.from_numpy(flows).to("cuda")
    geom = (c["w"], c["h"], c["pw"], c["ph"])
    expect, ranks = 0, []
    for r, sh in enumerate(shards):
        band = ebo.band_plan(ih, bounds, r, halo)
        for k in range(n_windows):
            ev = evs[k]
            p = cc.patch_of(ev["x"], ev["y"], geom)
            for u in sh["my"]:
                e = ev[p == u]
                if len(e) == 0:
                    continue
                reach = float(np.abs(t_ref[k] - e["t_us"]).max()) * abs(c["scale"]) * abs(flows[k, u, 1]) + 1.0
                above = band.band_row0 == 0 or e["y"].min() - reach >= band.band_row0 - 0.5
                below = band.band_row1 == ih or e["y"].max() + reach <= band.band_row1 - 0.5
                expect |= int(not (above and below))
        mk = lambda rows: torch.full((n_windows, rows, iw), -7, dtype=torch.int32, device="cuda") if rows else None
        R = dict(band=band, top=mk(band.top_rows), own=mk(band.own_rows), bottom=mk(band.bottom_rows),
                 flag=torch.zeros(1, dtype=torch.int32, device="cuda"))
        ctx = ebo.Context(**_shard_kw(ebo, c, n_windows, len(sh["ev"])))
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.set_patches(sh["ev"], sh["offs"], sh["rects"])
        ptr = lambda t: t.data_ptr() if t is not None else 0
        ctx.count_image_band_device(n_windows, t_ref, d_flows.data_ptr(), band, ptr(R["top"]), ptr(R["own"]), ptr(R["bottom"]),
                                    R["flag"].data_ptr())
        ctx.synchronize()
        R["ctx"] = ctx
        ranks.append(R)
    torch.cuda.synchronize()
    escaped = max(int(R["flag"].item()) for R in ranks)
    assert escaped == expect == (0 if halo == 70 else 1)
    if not escaped:
        rows = []
        for r, R in enumerate(ranks):
            band = R["band"]
            above = ranks[r - 1]["bottom"] if r > 0 else None
            below = ranks[r + 1]["top"] if r + 1 < world else None
            img = torch.zeros((n_windows, band.own_rows, iw), dtype=torch.float64, device="cuda")
            ptr = lambda t: t.data_ptr() if t is not None else 0
            R["ctx"].band_finish_device(n_windows, band, ptr(R["own"]), ptr(above), ptr(below), img.data_ptr())
            R["ctx"].synchronize()
            rows.append(img.cpu().numpy())
        full = np.concatenate(rows, axis=1)
        assert np.array_equal(full, want), _where(full, want)
    for R in ranks:
        R["ctx"].close()


@pytest.mark.parametrize("mode,impl", [(1, 0), (1, 1), (1, 3), (1, 4), (1, 5), (2, 0), (2, 1), (2, 3), (0, 2)])
def test_pileups_at_the_limits_of_the_packed_counters(ebo_ab, orc, monkeypatch, mode, impl):
    """One pixel collects 65535 events in the low and in the high half of its dword (the whole window: 16-bit counters,
    full), 65535 with five more on the other half and 65536 and 70000 (32-bit counters) -- from another patch, band and
    tile in the warped and field modes.  Bands of 1 KB: 8 rows of 16-bit counters, 4 of 32-bit."""
    for n, parity, extra in cc.PILE_VARIANTS:
        c, (x, y), (a, b) = cc.pileup(mode, n, parity, extra)
        want = oracle_images(orc, c)
        assert want[0, y, x] == a and want[0, y, x ^ 1] == b
        _check_forced(ebo_ab, orc, monkeypatch, c, impl, lds_kb=1)


@pytest.mark.parametrize("tile", [(16, 12), (24, 18)], ids=["interior", "first_column"])
@pytest.mark.parametrize("variant", cc.TILE_LIMIT_VARIANTS)
def test_tiles_16_bit_rule_at_its_edge(ebo_ab, orc, monkeypatch, variant, tile):
    """k_count_tiles counts a tile with 16-bit counters while nx * ny * maxEvents < 65536: 9 x 7281 = 65529 events on one
    pixel is the most that rule admits, 9 x 7282 and a far unit whose reach makes nx = ny = 5 take the 32-bit half-tile
    slices.  The pixel lies inside a 16 x 12 tile, and on the first column and row of a 24 x 18 one."""
    c, (x, y), n = cc.tile_limit(variant)
    assert (x % tile[0] == 0) == (tile == (24, 18))
    assert oracle_images(orc, c)[0, y, x] == n
    _check_forced(ebo_ab, orc, monkeypatch, c, 5, tile=tile)


_STORE = [(1, 1), (1, 3), (1, 4), (2, 1), (2, 3), (0, 2), (1, 5), (1, None), (2, None), (0, None)]


@pytest.mark.parametrize("mode,impl", _STORE)
def test_store_forms(ebo_ab, orc, monkeypatch, mode, impl):
    """61 x 43 pixels, three windows with a pattern each, bands of an odd number of rows: the 16-byte double2 stores, the
    odd-pixel tail (fed: the last pixel of every row counts events) and the scalar stores of a band or window that starts 8
    bytes off a 16-byte boundary.  Then the same image through ebo_count_image_device into a buffer at offset 0 and at + 8
    bytes: the same bits, and the doubles before and after the image untouched."""
    import torch
    c = cc.store_pattern(mode)
    kb = cc.STORE_LDS_KB.get(impl, 0)
    want = oracle_images(orc, c)
    _check_forced(ebo_ab, orc, monkeypatch, c, impl if impl is not None else 0, lds_kb=kb)
    n = want.size
    guard = 64
    with _context(ebo_ab, c) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.set_windows(c["ev"], c["offsets"])
        _force(monkeypatch, impl, lds_kb=kb)
        aux, d_aux = None, 0
        if mode == 1:
            aux = torch.from_numpy(np.ascontiguousarray(c["flows"])).to("cuda")
        elif mode == 2:
            aux = torch.from_numpy(np.ascontiguousarray(c["field"])).to("cuda")
        if aux is not None:
            d_aux = aux.data_ptr()
        for shift in (0, 1):
            buf = torch.full((guard + n + 1 + guard,), -3.0, dtype=torch.float64, device="cuda")
            assert buf.data_ptr() % 16 == 0
            ctx.count_image_device(mode, d_aux, buf.data_ptr() + 8 * (guard + shift))
            ctx.synchronize()
            host = buf.cpu().numpy()
            img = host[guard + shift:guard + shift + n].reshape(want.shape)
            assert np.array_equal(img, want), (mode, impl, shift, _where(img, want))
            assert (host[:guard + shift] == -3.0).all() and (host[guard + shift + n:] == -3.0).all()
