"""The evaluator's result lines, character for character: the reference's four (code/base/alignment.py:64-73), the two
Sinkhorn ones of the same shape, and what greedy_alignment's arguments select.  The literals are the format strings that
print_results held before it built its line from parts."""
import pytest

TOP_K, HITS, MR, MRR, COST = [1, 5, 10], [12.345, 50.0, 99.9], 123.45678, 0.0123456789, 1.23456

LINES = [
    (True, 10, None, "accurate results with csls: csls={}, hits@{} = {}%, mr = {:.3f}, mrr = {:.6f}, time = {:.3f} s ".format(10, TOP_K, HITS, MR, MRR, COST)),
    (True, 0, None, "accurate results: hits@{} = {}%, mr = {:.3f}, mrr = {:.6f}, time = {:.3f} s ".format(TOP_K, HITS, MR, MRR, COST)),
    (False, 10, None, "quick results with csls: csls={}, hits@{} = {}%, time = {:.3f} s ".format(10, TOP_K, HITS, COST)),
    (False, 0, None, "quick results: hits@{} = {}%, time = {:.3f} s ".format(TOP_K, HITS, COST)),
    (True, 0, (5, 0.05), "accurate results with sinkhorn: iters={}, tau={}, hits@{} = {}%, mr = {:.3f}, mrr = {:.6f}, time = {:.3f} s ".format(5, 0.05, TOP_K, HITS, MR, MRR, COST)),
    (False, 0, (5, 0.05), "quick results with sinkhorn: iters={}, tau={}, hits@{} = {}%, time = {:.3f} s ".format(5, 0.05, TOP_K, HITS, COST)),
    # sinkhorn wins over a csls_k that the callers never pass with it; a negative csls_k is no CSLS
    (True, 10, (1, 2.0), "accurate results with sinkhorn: iters=1, tau=2.0, hits@[1, 5, 10] = [12.345, 50.0, 99.9]%, mr = 123.457, mrr = 0.012346, time = 1.235 s "),
    (False, -1, None, "quick results: hits@[1, 5, 10] = [12.345, 50.0, 99.9]%, time = 1.235 s "),
    (True, 3, None, "accurate results with csls: csls=3, hits@[1, 5, 10] = [12.345, 50.0, 99.9]%, mr = 123.457, mrr = 0.012346, time = 1.235 s "),
]


@pytest.mark.parametrize("accurate,csls_k,sinkhorn,want", LINES)
def test_print_results_lines(capsys, accurate, csls_k, sinkhorn, want):
    from multike_amd.base.alignment import print_results
    print_results(TOP_K, HITS, MR, MRR, COST, accurate, csls_k, sinkhorn)
    assert capsys.readouterr().out == want + "\n"


def test_print_results_with_numpy_hits(capsys):
    """greedy_alignment hands a rounded NumPy array over: its str() is part of the line."""
    import numpy as np
    from multike_amd.base.alignment import print_results
    hits = np.round(np.array([1.0, 2.5, 3.0]) / 3 * 100, 3)
    print_results([1, 5, 10], hits, 2.0, 0.5, 0.25, True)
    assert capsys.readouterr().out == "accurate results: hits@[1, 5, 10] = {}%, mr = 2.000, mrr = 0.500000, time = 0.250 s \n".format(hits)
