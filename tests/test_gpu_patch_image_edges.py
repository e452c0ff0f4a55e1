"""k_patch_integrate (one workgroup of 256 per patch, signed counts in an LDS tile) and its two entries at their edges,
on the hand-built patches of tests/plumbing_cases.py: every image equals the oracle's as float64 bits, `updated`,
current_ts and time_last_update as integers.  Non-square and one-pixel-wide rects, images of exactly 16384 pixels, the
rings just inside and just outside fractional and negative corners, pile-ups on one pixel, empty patches in a batch,
nabla_offsets with gaps and in descending order (every word outside the images stays the caller's), round-half-to-even
ties and R6's time test at its boundaries.  Sizes the entries refuse are asserted by status alone: nothing is
launched for them.  tests/test_plumbing_cases_cpu.py shows on the CPU that each scene reaches its edge."""
import numpy as np
import pytest

import plumbing_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(ebo):
    with ebo.Context(image_w=240, image_h=180) as c:
        yield c


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def oracle_plain(orc, patches):
    """-> (images, current_ts, time_last_update) per patch; an empty patch: a zero image and None stamps."""
    out = []
    for ev, rect in patches:
        if len(ev):
            out.append(orc.patch_integrate(ev, rect))
        else:
            out.append((np.zeros((int(rect[3]), int(rect[2]))), None, None))
    return out


def run_plain(ebo, ctx, patches, noff=None, length=None, stamp=-777):
    """One ebo_patch_integrate call on a guard-filled buffer -> (buffer, offsets, current_ts, time_last_update)."""
    ev, off, rects = K.pack_patches(patches)
    sizes = [int(r[2]) * int(r[3]) for r in rects]
    if noff is None:
        noff = np.asarray([sum(sizes[:i]) for i in range(len(sizes))], dtype=np.uint64)
        length = int(sum(sizes))
    nabla = np.full(length, K.GUARD)
    cur = np.full(len(patches), stamp, dtype=np.int64)
    last = np.full(len(patches), stamp, dtype=np.int64)
    rc = K.raw_patch_integrate(ebo, ctx, ev, off, rects, noff, nabla, cur, last)
    assert rc == 0, ebo.lib().ebo_last_error(ctx._h)
    return nabla, [int(o) for o in noff], cur, last


def assert_plain(ebo, ctx, orc, patches, **kw):
    nabla, noff, cur, last = run_plain(ebo, ctx, patches, **kw)
    rest = np.ones(len(nabla), dtype=bool)
    for i, (img, ocur, olast) in enumerate(oracle_plain(orc, patches)):
        got = nabla[noff[i]:noff[i] + img.size]
        assert np.array_equal(bits(got), bits(img.ravel())), i
        rest[noff[i]:noff[i] + img.size] = False
        if ocur is None:   # an empty patch: its entries are left as the caller had them
            assert cur[i] == -777 and last[i] == -777, i
        else:
            assert cur[i] == ocur and last[i] == olast, i
    assert np.all(bits(nabla[rest]) == bits(K.GUARD)), "a word outside the images changed"


@pytest.mark.parametrize("scene", ["nonsquare", "limit", "border", "pileup", "batch_with_empty"])
def test_patch_images_match_the_oracle(ebo, ctx, orc, scene):
    assert_plain(ebo, ctx, orc, getattr(K, "patches_" + scene)())


@pytest.mark.parametrize("layout", ["gaps", "descending", "descending_dense"])
def test_patch_integrate_writes_only_its_images(ebo, ctx, orc, layout):
    patches = K.patches_batch_with_empty() + K.patches_border()[:2]
    sizes = [int(p[1][2]) * int(p[1][3]) for p in patches]
    noff, length = K.offset_layouts(sizes)[layout]
    assert_plain(ebo, ctx, orc, patches, noff=np.asarray(noff, dtype=np.uint64), length=length)


def run_mc(ebo, ctx, patches, init, noff):
    ev, off, rects = K.pack_patches(patches)
    traj, mid = K.pack_traj(patches)
    nabla = init.copy()
    upd = np.full(len(patches), -9, dtype=np.int32)
    rc = K.raw_patch_integrate_mc(ebo, ctx, ev, off, rects, traj, mid, noff, nabla, upd)
    assert rc == 0, ebo.lib().ebo_last_error(ctx._h)
    return nabla, upd


def assert_mc(ebo, ctx, orc, patches, noff=None, length=None):
    """init= is a pattern that differs at every word: a failing patch's image, and every word outside the images, comes
    back bit for bit; a passing patch's image is the oracle's, zeros included."""
    sizes = [int(p[1][2]) * int(p[1][3]) for p in patches]
    if noff is None:
        noff, length = [sum(sizes[:i]) for i in range(len(sizes))], sum(sizes)
    init = K.GUARD + np.arange(length, dtype=np.float64)
    nabla, upd = run_mc(ebo, ctx, patches, init, np.asarray(noff, dtype=np.uint64))
    want = init.copy()
    for i, (ev, rect, pre, last, mid) in enumerate(patches):
        img, passed = (orc.patch_integrate_mc(ev, rect, pre, last, mid) if len(ev) else (None, False))
        assert upd[i] == int(passed), i
        if passed:
            want[noff[i]:noff[i] + sizes[i]] = img.ravel()
    assert np.array_equal(bits(nabla), bits(want))
    return upd


def test_patch_mc_rounds_half_to_even(ebo, ctx, orc):
    upd = assert_mc(ebo, ctx, orc, [K.patch_mc_ties()])
    assert upd.tolist() == [1]


def test_patch_mc_time_test_boundaries_and_init(ebo, ctx, orc):
    patches = K.patches_mc_time()
    empty = (K.events([], []), (0.0, 0.0, 3.0, 3.0), K.MC_PRE, K.MC_LAST, K.MC_MID)   # no events: fails, untouched
    upd = assert_mc(ebo, ctx, orc, patches + [empty])
    assert upd.tolist() == [int(p) for _, p in K.MC_TIME_TESTS] + [0]


@pytest.mark.parametrize("layout", ["gaps", "descending", "descending_dense"])
def test_patch_integrate_mc_writes_only_its_images(ebo, ctx, orc, layout):
    patches = K.patches_mc_time()[:5] + [K.patch_mc_ties()]
    sizes = [int(p[1][2]) * int(p[1][3]) for p in patches]
    noff, length = K.offset_layouts(sizes)[layout]
    assert_mc(ebo, ctx, orc, patches, noff=noff, length=length)


def test_patch_mc_time_step_outside_int32_is_refused(ebo, ctx):
    pre, last, mid = K.MC_RANGE
    patches = [(K.patch_distinct(K.TIME_RECT), K.TIME_RECT, pre, last, mid)]
    ev, off, rects = K.pack_patches(patches)
    traj, m = K.pack_traj(patches)
    nabla = np.full(20, K.GUARD)
    upd = np.zeros(1, dtype=np.int32)
    rc = K.raw_patch_integrate_mc(ebo, ctx, ev, off, rects, traj, m, np.zeros(1, dtype=np.uint64), nabla, upd)
    assert rc == ebo.ERR_RANGE
    assert np.all(bits(nabla) == bits(K.GUARD))


@pytest.mark.parametrize("rect,status", K.REFUSED, ids=["%gx%g" % r[0][2:] for r in K.REFUSED])
@pytest.mark.parametrize("where", ["alone", "last_of_three"])
def test_patch_sizes_the_entries_refuse(ebo, ctx, rect, status, where):
    """A status and nothing else: refused before anything is copied or launched, so the caller's nabla, stamps and
    `updated` are as they were -- also when admitted patches come before the refused one."""
    assert (status == ebo.ERR_ARG) == (not np.isfinite(rect[2:]).all() or rect[2] % 1 != 0 or rect[3] % 1 != 0)
    good = (K.patch_distinct(K.TIME_RECT), K.TIME_RECT)
    some = K.events([int(rect[0])], [int(rect[1])])
    plain = [good, good, (some, rect)] if where == "last_of_three" else [(some, rect)]
    ev, off, rects = K.pack_patches(plain)
    noff = np.arange(len(plain), dtype=np.uint64) * 40
    nabla = np.full(40 * len(plain) + 70000, K.GUARD)
    cur = np.full(len(plain), -777, dtype=np.int64)
    last = np.full(len(plain), -777, dtype=np.int64)
    assert K.raw_patch_integrate(ebo, ctx, ev, off, rects, noff, nabla, cur, last) == status
    assert np.all(bits(nabla) == bits(K.GUARD)) and np.all(cur == -777) and np.all(last == -777)
    mc = [p + (K.MC_PRE, K.MC_LAST, 1005) for p in plain]
    traj, mid = K.pack_traj(mc)
    upd = np.full(len(plain), -9, dtype=np.int32)
    assert K.raw_patch_integrate_mc(ebo, ctx, ev, off, rects, traj, mid, noff, nabla, upd) == status
    assert np.all(bits(nabla) == bits(K.GUARD)) and np.all(upd == -9)
