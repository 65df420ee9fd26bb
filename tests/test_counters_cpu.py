"""capi.read_counters, the one reader behind the counter methods of capi.Context and pipeline.Store, against a fake C
getter that writes known values through its pointers.  No device."""
import ctypes as C

import pytest

from sina_amd import capi, pipeline


def _fake_getter(rc, seen):
    """int f(void *handle, double *ms, uint64_t *a, uint64_t *b) as a C function: 1.5, 7 and 2^40 + 3 through the pointers"""
    @C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), capi.u64p, capi.u64p)
    def f(handle, ms, a, b):
        seen.append(handle)
        ms[0], a[0], b[0] = 1.5, 7, (1 << 40) + 3
        return rc
    return f


FIELDS = capi.KERNEL_MS + capi.u64_fields("sequences", "pairs")


def test_the_dict_has_the_fields_order_and_types():
    seen, codes = [], []
    d = capi.read_counters(_fake_getter(0, seen), (C.c_void_p(0x1234),), FIELDS, codes.append)
    assert seen == [0x1234] and codes == [0]
    assert list(d.items()) == [("kernel_ms", 1.5), ("sequences", 7), ("pairs", (1 << 40) + 3)]
    assert [type(v) for v in d.values()] == [float, int, int]
    # the order is the fields', not the types': an integer in front of the time, as the store's getters have it
    swapped = capi.u64_fields("sequences") + capi.KERNEL_MS

    @C.CFUNCTYPE(C.c_int, capi.u64p, C.POINTER(C.c_double))
    def g(a, ms):
        a[0], ms[0] = 9, 0.25
        return 0
    assert list(capi.read_counters(g, (), swapped, codes.append).items()) == [("sequences", 9), ("kernel_ms", 0.25)]


def test_a_failing_getter_reaches_the_checker():
    class Refused(Exception):
        pass

    def check(rc):
        if rc != 0:
            raise Refused(rc)
    with pytest.raises(Refused) as e:
        capi.read_counters(_fake_getter(3, []), (None,), FIELDS, check)
    assert e.value.args == (3,)


def test_the_methods_it_serves_keep_their_names():
    for name in ("match_stats", "rank_stats", "pair_stats", "pair_inplace_stats", "identity_inplace_stats", "wide_queries",
                 "long_queries", "big_select_queries"):
        assert callable(getattr(capi.Context, name)), name
    for name in ("match_stats", "rank_stats", "pair_stats", "pair_inplace_stats", "identity_inplace_stats", "slow_path_queries",
                 "big_select_queries"):
        assert callable(getattr(pipeline.Store, name)), name
