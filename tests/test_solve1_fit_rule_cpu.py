"""CPU: the host part of the one-launch kernel's admission rule and its size classes (hipsdp_solve1_fits / hipsdp_solve1_class of the
units library, wrapping hs_solve1_fits of csrc/solve1_body.h and hs_solve1_class of csrc/solve1.hip).  No device is touched.  The GPU
tests of tests/test_gpu_solve1_oracle.py pick their shapes from the same rule."""


def test_one_launch_fit_rule_and_size_classes(hb):
    """the host part of the one-launch kernel's admission rule (hipsdp_solve1_fits of the units library): the largest blocks it admits
    (no LP rows) - one, two, eight blocks at m = 1, 64, 108, 128 - and the kernel instance that serves a shape"""
    def largest(m, q, k):
        return max([n for n in range(1, 65) if hb.solve1_fits(m, q, [n] * k)], default=0)
    assert [largest(1, 0, k) for k in (1, 2, 8)] == [49, 34, 16]
    assert [largest(64, 0, k) for k in (1, 2, 8)] == [41, 29, 13]
    assert [largest(108, 0, k) for k in (1, 2, 8)] == [37, 25, 12]
    assert [largest(128, 0, k) for k in (1, 2, 8)] == [32, 22, 10]
    assert [largest(64, 200, k) for k in (1, 2, 8)] == [38, 27, 13]
    # outside the rule's domain: no blocks, more than 8 blocks, m above 128, q above 4096, a block of 65 rows
    assert not hb.solve1_fits(129, 0, [4]) and not hb.solve1_fits(1, 4097, [4]) and not hb.solve1_fits(1, 0, [65])
    assert not hb.solve1_fits(1, 0, []) and not hb.solve1_fits(1, 0, [2] * 9)
    assert [hb.solve1_class(64, ns) for ns in ([10] * 8, [11], [3, 16], [17])] == [10, 16, 16, 64]
    assert hb.solve1_class(65, [3]) == 1064 and hb.solve1_class(1, []) == -1
