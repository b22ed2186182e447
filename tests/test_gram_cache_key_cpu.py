"""CPU test of the host bookkeeping of the cold-start store (csrc/hs_gram_cache.h) through the host-only entries of the units library:
generation numbers are never handed out twice, and a stored Gram matrix serves exactly the solves whose key equals its own in every
field - the matrices' generations, the shape, the identity form of each block and the workspace the Gram kernel summed in."""
import ctypes as C

import pytest

FULL, PACKED = 1, 2
WS = (64 * 121 * 121, 121, 1)            # kws_len, chunk_cols, full


@pytest.fixture(scope="module")
def ulib(hb):
    u = hb.ulib()
    u.hipsdp_gram_gen_next.restype = C.c_ulonglong
    return u


def match(ulib, a, b):
    def args(k):
        m, ns, forms, gens, ws = k
        nb = len(ns)
        return [C.c_int(m), C.c_int(nb), (C.c_int * max(nb, 1))(*ns), (C.c_int * max(nb, 1))(*forms),
                (C.c_ulonglong * max(nb, 1))(*gens), (C.c_longlong * 3)(*ws)]
    return ulib.hipsdp_gram_key_match_unit(*(args(a) + args(b)))


def test_generation_numbers_only_grow(ulib):
    c = C.c_ulonglong(0)
    seen = [ulib.hipsdp_gram_gen_next(C.byref(c)) for _ in range(1000)]
    assert seen == list(range(1, 1001)) and c.value == 1000          # 0 is never handed out: it means "never written"
    c = C.c_ulonglong(2 ** 63)
    assert ulib.hipsdp_gram_gen_next(C.byref(c)) == 2 ** 63 + 1
    assert ulib.hipsdp_gram_gen_next(None) == 0


def test_key_matches_itself_and_nothing_else(ulib):
    key = (120, [65, 70], [PACKED, FULL], [3, 4], WS)
    assert match(ulib, key, key) == 1
    m, ns, forms, gens, ws = key
    different = [
        (121, ns, forms, gens, ws),                                   # another number of variables
        (m, [65, 71], forms, gens, ws),                               # another block size
        (m, [70, 65], [FULL, PACKED], [4, 3], ws),                    # the same blocks in another order: another summation order
        (m, ns, [FULL, FULL], gens, ws),                              # another identity form
        (m, ns, forms, [3, 5], ws),                                   # a block was written
        (m, ns, forms, [5, 4], ws),
        (m, [65], [PACKED], [3], ws),                                 # fewer blocks
        (m, ns, forms, gens, (WS[0] // 2, WS[1], WS[2])),             # fewer slabs: another summation
        (m, ns, forms, gens, (WS[0], 128, WS[2])),
        (m, ns, forms, gens, (WS[0], WS[1], 0)),
    ]
    for other in different:
        assert match(ulib, key, other) == 0 and match(ulib, other, key) == 0, other
        assert match(ulib, other, other) == 1, other


def test_keys_the_store_does_not_take(ulib):
    """no blocks, more blocks than a key holds, a generation of 0 (never written), a form that is none: such a key matches nothing, not
    even itself - the solve computes"""
    bad = [
        (120, [], [], [], WS),
        (120, [65] * 65, [PACKED] * 65, list(range(1, 66)), WS),
        (120, [65], [PACKED], [0], WS),
        (120, [65], [0], [3], WS),
        (120, [65], [3], [3], WS),
        (120, [0], [PACKED], [3], WS),
        (-1, [65], [PACKED], [3], WS),
    ]
    good = (120, [65], [PACKED], [3], WS)
    for k in bad:
        assert match(ulib, k, k) == 0 and match(ulib, k, good) == 0 and match(ulib, good, k) == 0, k
    assert match(ulib, (120, [65] * 64, [PACKED] * 64, list(range(1, 65)), WS), (120, [65] * 64, [PACKED] * 64, list(range(1, 65)), WS)) == 1


def test_write_then_write_back_is_still_a_new_generation(ulib):
    """the bump-on-write rule as the engine applies it (a_written): store under the current generations, write a block, and the key no
    longer matches - nor after any number of further writes, whatever they wrote"""
    c = C.c_ulonglong(0)
    gens = [ulib.hipsdp_gram_gen_next(C.byref(c)), ulib.hipsdp_gram_gen_next(C.byref(c))]
    stored = (120, [65, 70], [PACKED, PACKED], list(gens), WS)
    assert match(ulib, stored, (120, [65, 70], [PACKED, PACKED], list(gens), WS)) == 1
    for _ in range(5):
        gens[1] = ulib.hipsdp_gram_gen_next(C.byref(c))
        assert match(ulib, stored, (120, [65, 70], [PACKED, PACKED], list(gens), WS)) == 0
