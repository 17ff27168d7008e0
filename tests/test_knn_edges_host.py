"""CPU tests that pin the KNN edge references and case generators of tests/knn_ref.py without a GPU: the NumPy `lexsort`
and the torch form of the promised result agree, the float32 reference itself keeps the derived value bound against float64,
and every generator's asserted property holds at the sizes tests/test_knn_edges.py uses."""
import numpy as np
import pytest
import torch

from tests import knn_ref as kr

CLASS_NAMES = sorted(kr.CLASSES)
CLASS_M = (257, 4097)                    # tests/test_knn_edges.py: every class of the table
SEAM_M = (1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3072, 3073, 4095, 4096, 4097, 8193)


def _small(name):
    return kr.make_case(name, 10 if name == "overflow" else 257)


@pytest.mark.parametrize("name", CLASS_NAMES)
def test_numpy_lexsort_and_torch_forms_agree(name):
    for case in (_small(name), kr.make_case(name, 600)):
        x = case.points
        M = x.size(0)
        for K, excl in ((min(32, M), False), (min(32, M - 1), True), (3, True)):
            ti, td = kr.exhaustive_f32(x, x, K, excl, chunk=100)
            ni, nd = kr.exhaustive_f32_numpy(x.numpy(), x.numpy(), K, excl)
            assert np.array_equal(ti.numpy(), ni) and np.array_equal(td.numpy().view(np.int32), nd.view(np.int32)), (name, M, K, excl)
    # free queries: not the references, fewer rows than references
    q = torch.from_numpy(np.random.default_rng(1).random((37, 3)).astype(np.float32) * 6 - 3)
    ti, td = kr.exhaustive_f32(q, x, 8)
    ni, nd = kr.exhaustive_f32_numpy(q.numpy(), x.numpy(), 8)
    assert np.array_equal(ti.numpy(), ni) and np.array_equal(td.numpy().view(np.int32), nd.view(np.int32))


@pytest.mark.parametrize("name", CLASS_NAMES)
def test_float32_reference_keeps_the_value_bound(name):
    for case in (_small(name), kr.make_case(name, 1025)):
        x = case.points
        M = x.size(0)
        for K, excl in ((min(32, M), False), (min(32, M - 1), True)):
            _, d2 = kr.exhaustive_f32(x, x, K, excl)
            bad = kr.value_bound_violations(d2, kr.exhaustive_f64(x, x, K, excl))
            assert not bool(bad.any()), (name, M, K, excl, int(bad.sum()))


def test_value_bound_rejects_what_it_should():
    d64 = torch.tensor([[1.0, 4.0, 1e39, 1e39, 0.0, 0.0]], dtype=torch.float64)
    ok = torch.tensor([[1.0, 4.0 * (1 + 2.0 ** -22), float("inf"), float("inf"), 0.0, 2.0 ** -126]])
    assert not bool(kr.value_bound_violations(ok, d64).any())
    bad = torch.tensor([[1.0 + 2.0 ** -20, float("nan"), 3.4e38, float("-inf"), 1e-37, float("inf")]])
    assert bool(kr.value_bound_violations(bad, d64).all())


@pytest.mark.parametrize("name", CLASS_NAMES)
def test_generator_properties_at_the_class_sizes(name):
    for M in CLASS_M + ((10,) if name == "overflow" else ()):
        case = kr.make_case(name, M)
        assert case.points.shape == (M, 3) and case.points.dtype == torch.float32 and bool(torch.isfinite(case.points).all())
        case.check()
        assert torch.equal(kr.make_case(name, M).points, case.points), "seeded"


@pytest.mark.parametrize("M", SEAM_M)
def test_generator_properties_at_the_seam_sizes(M):
    for name in ("uniform", "lattice"):
        case = kr.make_case(name, M)
        assert case.points.shape == (M, 3)
        case.check()


def test_repeats_and_lattice_at_the_free_query_sizes():
    kr.make_case("repeats", 4097).check()
    c = kr.make_case("lattice", 1025)
    c.check()
    assert len(np.unique(c.points.numpy(), axis=0)) == 1025


def test_overflow_reference_stays_in_range():
    """the answer the search owes for finite inputs whose float32 distances overflow: indices in [0, M), the infinite ones by index"""
    for M in (10, 257):
        x = kr.make_case("overflow", M).points
        assert float((x[:, 0].max() - x[:, 0].min()) ** 2) == float("inf")
        for K, excl in ((8, False), (8, True), (3, True)):
            i, d = kr.exhaustive_f32(x, x, K, excl)
            assert bool(((i >= 0) & (i < M)).all()) and bool((d[:, 1:] >= d[:, :-1]).all())
            tied = d[:, 1:] == d[:, :-1]
            assert bool((i[:, 1:][tied] > i[:, :-1][tied]).all())
        assert bool(torch.isinf(kr.exhaustive_f32(x, x, 8)[1]).any())


def test_morton_restatement_on_known_points():
    p = np.array([[0, 0, 0], [1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.5, 0.5]], np.float32)
    c = kr.morton_codes(p)
    assert c[0] == 0 and c[1] == 0x3FFFFFFF and c[2] == 0x09249249 and c[3] == 0x12492492 and c[4] == 0x24924924
    assert c[5] == sum(((511 >> b) & 1) * (7 << (3 * b)) for b in range(10))
    far = kr.morton_codes(np.array([[-9, -9, -9], [9, 9, 9]], np.float32), p)      # queries outside the box clamp to its faces
    assert far[0] == 0 and far[1] == 0x3FFFFFFF
