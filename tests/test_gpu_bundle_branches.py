"""GPU: the branches of B9 and the options that tests/test_gpu_bundle.py never takes, against tests/bundle_ref.py under
that module's rule: iterations, num_evals_*, termination and the trace's flags as equal integers, every double (poses,
points, initial and final cost, trace) within 10 x the scene's delta (the restatement against itself with every stated
sum reversed; computed here, in the module's fixture), the count of bit-equal doubles printed.  EVERY field of a
scene's options reaches the kernel.  tests/test_bundle_cpu.py checks on the CPU that each scene takes the branch it is
here for, that none of its decisions is a coin toss in either sum order, and that the device's text compiled for the
host gives the same: a fault found here can be looked for there.

rej_mrd, nonmono_m5, nonmono_m2, ptol4, noscale_clip and ftol3 are there because no other scene varies
min_relative_decrease, max_consecutive_nonmonotonic, parameter_tolerance, function_tolerance (other than to 0) or makes
jacobi_scaling matter: with the option replaced by its default in the kernel's text, every other scene still passes.

Scenes (bundle_ref.branch_scenes; Huber 0.8, camera B.CAM; options other than those named are the defaults; a is
scene(1, 3, 4)) and their delta as measured on the CPU.  Trace flags: A taken, R rejected, I invalid, C converged at
this candidate.
  rej          4 frames, 30 points, 0.3 px noise, 10 % outliers, a far start: 34 iterations, ARRA..AC: the
               rejected step's radius / decrease, and the old Jacobian, U, g, W, res used again                1.1e-8
  rej_mrd      rej with min_relative_decrease 0.5 (the closest quality is 0.4911): steps rej takes are
               rejected, ARRRAAAAAARRRA..AC, 40 iterations                                                     3.3e-9
  rej4         3 frames, 12 points, a very far start, initial_radius 1e16: four rejections in a row at
               iterations 8-11 (decrease 2, 4, 8, 16), 32 iterations                                           5.5e-7
  nonmono      the same with use_nonmonotonic: iteration 8 is taken although the cost rises from 40.1173 to
               40.1318; no rejection, 28 iterations                                                            6.5e-7
  nonmono_cut  the same cut at max_num_iterations 8: termination 1, and the point returned is iterate 7, the
               lowest-cost point visited, not the last                                                         1.4e-7
  nonmono_m5   another very far start (seed 68), initial_radius 1e16, use_nonmonotonic: ten rejections in a
               row (decrease up to 1024), then five steps taken that raise the cost; 35 iterations            4.3e-6
  nonmono_m2   the same with max_consecutive_nonmonotonic 2: the count of steps without a new minimum
               reaches its limit and is reset several times, the reference cost moves, rejections come
               back (R x 10, A x 16, RRRR, A x 9, RRRR, AAAC): 47 iterations                                   4.3e-6
  invalid      the edge scene with min_lm_diagonal 0: its free frame without observations has a pivot of
               exactly 0, so IIIII, termination 2 without one cost evaluation, radii 5000 .. 312.5             0
  invalid3     the same with max_consecutive_invalid 3: III                                                    0
  minrad       a with initial_radius 1e-33 < min_radius: 0 iterations, termination 0                           0
  gtol         a with function_tolerance 0, parameter_tolerance 0, gradient_tolerance 1e-6: AAAA, ends by
               the gradient, no flag-2 row                                                                     2.4e-11
  ptol         a with function_tolerance 0, gradient_tolerance 0: AAAAC by the step norm                       2.4e-11
  ptol4        the same with parameter_tolerance 1e-4: AAC                                                     1.1e-15
  maxrad       a with max_radius 2e4, function_tolerance 0: the radius is held at 2e4, AAAAAC                  5.1e-9
  lmclip       a with min_lm_diagonal = max_lm_diagonal = 0.1, initial_radius 1: both clips of B7's
               damping on every diagonal, 9 iterations                                                         1.5e-11
  noscale      a with jacobi_scaling 0: AAAAC (B7 damps by the diagonal itself, so this path is a's but for
               roundings)                                                                                      2.9e-11
  noscale_clip lmclip with jacobi_scaling 0: with the damping clipped to a constant the scaling decides
               the path, 5 iterations instead of 9                                                             1.4e-11
  ftol3        rej with function_tolerance 1e-3: ends by the cost change alone at iteration 15                 4.3e-11
  fix24        fix_points with 24 free frames, 60 points seen by 3..24, N = 847: the block-diagonal reduced
               system at dim = 144, AAAAC                                                                      1.7e-9
  dense24      24 frames, 30 points, every point in every frame (N = 720): no empty block in the reduced
               system, dim = 132, AAAAAC                                                                       9.6e-10
  big          16 frames, 4096 points, 65535 observations (both limits), max_num_iterations 2: AA,
               termination 1; every lane strides 256 times and the work offsets are at their largest           6.0e-15
Device time of big on an MI355X (a process's first call of that shape, one workgroup, two iterations), two runs: 139 and
147 ms for the kernel, 144 and 152 ms for the whole call; the test prints both for every scene at every run.
"""
import numpy as np
import pytest

import bundle_ref as B
from bundle_check import check, same, same_result

pytestmark = pytest.mark.gpu

# written out so that a test's id names its scene; the fixture checks that it is all of branch_scenes()
NAMES = ["rej", "rej_mrd", "rej4", "nonmono", "nonmono_cut", "nonmono_m5", "nonmono_m2", "invalid", "invalid3", "minrad", "gtol", "ptol",
         "ptol4", "maxrad", "lmclip", "noscale", "noscale_clip", "ftol3", "fix24", "dense24", "big"]


@pytest.fixture(scope="module")
def scenes():
    out = B.branch_scenes()
    assert sorted(out) == sorted(NAMES)
    return out


@pytest.fixture(scope="module")
def refs(scenes):
    """name -> (the restatement's result, delta); computed once."""
    out = {}
    for name, (pr, fix, o) in scenes.items():
        fwd = B.solve(pr, B.HUBER, fix, o)
        out[name] = (fwd, B.result_difference(fwd, B.solve(pr, B.HUBER, fix, o, reverse_sums=True)))
    return out


def run(ebo, c, problems, fix, o):
    """One call: the problems share fix_points and the options, every field of which is handed over."""
    assert set(o) == {f for f, _ in ebo.SolverOpts._fields_} - {"mode"}
    return c.bundle_adjust(problems, B.CAM, B.HUBER, fix_points=fix, opts=ebo.default_ba_opts(**o), trace=True)


@pytest.mark.parametrize("name", NAMES)
def test_scene_equals_the_restatement(ebo, scenes, refs, name):
    pr, fix, o = scenes[name]
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        c.two_view_timing(True)
        got = run(ebo, c, [pr], fix, o)[0]
        ms = c.two_view_timing(False)
    print("%s: kernel %.3f ms, call %.3f ms" % (name, ms[0], ms[4]))
    check(name, got, refs)
    s = got["summary"]
    if name in ("invalid", "invalid3", "minrad"):                       # nothing moved: the inputs come back bit for bit
        assert same(got["poses"], pr["poses"]) and same(got["points"], pr["points"])
        assert same(s["final_cost"], s["initial_cost"])
    if name == "nonmono_cut":                                           # not the last iterate's cost
        assert s["final_cost"] < got["trace"][8, 0]
    if name == "fix24":
        assert same(got["points"], pr["points"])
        assert not any(same(got["poses"][k], pr["poses"][k]) for k in range(24))
    if name == "big":
        assert s["final_cost"] < s["initial_cost"]


@pytest.mark.parametrize("names, over", [
    (("a", "rej4", "a"), dict(initial_radius=1e16)),            # one that rejects four times between two that never do
    (("a", "invalid", "a"), dict(min_lm_diagonal=0.0)),         # one that leaves at termination 2 without a cost evaluation
    (("a", "big", "dense24"), dict(max_num_iterations=2)),      # the big one's work memory not at offset 0, one behind it
], ids=["rej4", "invalid", "big"])
def test_a_batch_that_diverges_equals_each_alone_and_itself(ebo, scenes, refs, names, over):
    """Problems of one call that take different branches: every result equal, bit for bit, to that of the problem alone
    under the same options and to a second run of the call."""
    o = B.default_opts(**over)
    prs = dict(scenes, a=(B.scene(1, 3, 4), False, None))
    assert scenes[names[1]][2] == o                                     # the middle one as the parametrised test runs it
    problems = [prs[n][0] for n in names]
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        batch = run(ebo, c, problems, False, o)
        again = run(ebo, c, problems, False, o)
        alone = {n: run(ebo, c, [prs[n][0]], False, o)[0] for n in set(names)}
    for n, g, h in zip(names, batch, again):
        assert same_result(g, alone[n]), n
        assert same_result(g, h), n
    check(names[1], batch[1], refs)
    flags = lambda g: g["trace"][1:g["summary"]["iterations"] + 1, 3]
    if names[1] != "big":                                               # they did go different ways: the neighbours only take steps
        assert (flags(batch[1]) <= 0.0).any() and all((flags(batch[k]) >= 1.0).all() for k in (0, 2))


@pytest.mark.parametrize("name", ["rej4", "fix24"])
def test_host_form_equals_device_form(ebo, scenes, name):
    import torch
    pr, fix, od = scenes[name]
    o = ebo.default_ba_opts(**od)
    of, op, uv = B.sort_observations(len(pr["poses"]), pr["of"], pr["op"], pr["uv"])
    fo, po, oo = (np.array([0, n], dtype=np.int32) for n in (len(pr["poses"]), len(pr["points"]), len(of)))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    d_poses, d_fixed, d_points = dev(pr["poses"].reshape(-1, 12)), dev(pr["fixed"].astype(np.uint8)), dev(pr["points"])
    d_of, d_op, d_uv = dev(of), dev(op), dev(uv)
    d_trace = torch.full((1, o.max_num_iterations + 1, 4), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        host = c.bundle_adjust([pr], B.CAM, B.HUBER, fix_points=fix, opts=o, trace=True)[0]
        summ = c.bundle_adjust_device(fo, po, oo, d_poses.data_ptr(), d_fixed.data_ptr(), d_points.data_ptr(), d_of.data_ptr(),
                                      d_op.data_ptr(), d_uv.data_ptr(), B.CAM, B.HUBER, fix_points=fix, opts=o, d_trace=d_trace.data_ptr())[0]
        got = dict(poses=d_poses.cpu().numpy().reshape(-1, 3, 4), points=d_points.cpu().numpy(), trace=d_trace.cpu().numpy()[0], summary=summ)
    assert same_result(got, host)
    assert host["summary"]["iterations"] > 0 and host["summary"]["termination"] == 0
