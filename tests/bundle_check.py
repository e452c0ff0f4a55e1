"""What tests/test_gpu_bundle.py and tests/test_gpu_bundle_branches.py share: bit equality of doubles and of whole
results, and the comparison of a device result with the restatement's (integers and trace flags equal, every double
within 10 x the scene's delta; the reason for that margin is in test_gpu_bundle.py's header)."""
import numpy as np

import bundle_ref as B

INTS = ("iterations", "num_evals_cost", "num_evals_jac", "termination")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def same_result(x, y):
    return (same(x["poses"], y["poses"]) and same(x["points"], y["points"]) and same(x["trace"], y["trace"]) and
            all(x["summary"][k] == y["summary"][k] for k in INTS) and
            same(x["summary"]["initial_cost"], y["summary"]["initial_cost"]) and same(x["summary"]["final_cost"], y["summary"]["final_cost"]))


def check(name, got, refs):
    """got against refs[name] = (the restatement's result, delta); -> (bit-equal doubles, doubles compared)."""
    want, delta = refs[name]
    for k in INTS:
        assert got["summary"][k] == want["summary"][k], (name, k, got["summary"], want["summary"])
    assert np.array_equal(got["trace"][:, 3], want["trace"][:, 3]), name
    pairs = [(got[k], want[k]) for k in ("poses", "points", "trace")] + \
            [(got["summary"][k], want["summary"][k]) for k in ("initial_cost", "final_cost")]
    equal = sum(int(((bits(a) == bits(b)) | (np.isnan(np.asarray(a, float)) & np.isnan(np.asarray(b, float)))).sum()) for a, b in pairs)
    total = sum(np.asarray(a).size for a, _ in pairs)
    worst = max(B.difference(a, b) for a, b in pairs)
    print("%s: %d of %d doubles bit-equal, largest difference %.3g, delta %.3g" % (name, equal, total, worst, delta))
    assert worst <= 10 * delta, (name, worst, delta)
    return equal, total
