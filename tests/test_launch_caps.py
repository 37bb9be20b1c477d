"""acmhip_device_set_launch_caps without a device: the check and the exchange are acm_kernel_geo.cpp's acmk_launch_caps_set (the setter
is that call under the handle's lock), and the five built-in numbers have one owner, include/acm_launch_caps.h."""
import ctypes as C
import os
import re

import pytest

from libacm_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [name for name, _ in capi.LaunchCaps._fields_]


def header_builtins():
    src = open(os.path.join(ROOT, "include", "acm_launch_caps.h")).read()
    out = {}
    for name, text in re.findall(r"^#define ACM_CAP_([A-Z_]+)\s+\(?([0-9u<> ]+?)\)?\s*(?:/\*.*)?$", src, flags=re.M):
        out[name.lower()] = eval(text.replace("u", ""))
    return out


def test_builtin_values_have_one_owner():
    """the header's numbers are the wrapper's, and no launcher or layout keeps a literal of its own beside them"""
    assert header_builtins() == capi.LAUNCH_CAPS_BUILTIN == {"list_slice": 65535, "small_grid_x": 4096, "parse_slice": 65535,
                                                             "parse_grid_x": 2048, "dense_grid": 1 << 20}
    struct = re.search(r"typedef struct acmhip_launch_caps \{(.*?)\} acmhip_launch_caps;", open(os.path.join(ROOT, "include", "acm_launch_caps.h")).read(),
                       flags=re.S).group(1)
    assert re.findall(r"uint32_t (\w+);", struct) == FIELDS and C.sizeof(capi.LaunchCaps) == 20
    csrc = os.path.join(ROOT, "libacm_amd", "csrc")
    text = {f: re.sub(r"/\*.*?\*/", "", open(os.path.join(csrc, f)).read(), flags=re.S) for f in ("acm_kernels.hip", "acm_parse.hip", "acm_dense_vec.h")}
    assert "SW_MAX_Y = ACM_CAP_LIST_SLICE" in text["acm_kernels.hip"] and "ACM_CAP_SMALL_GRID_X" in text["acm_kernels.hip"]
    assert "ACM_CAP_PARSE_SLICE" in text["acm_parse.hip"] and "ACM_CAP_PARSE_GRID_X" in text["acm_parse.hip"]
    assert "DENSE_MAX_GRID = ACM_CAP_DENSE_GRID" in text["acm_dense_vec.h"]
    assert "65535" not in text["acm_parse.hip"] and not re.search(r"gx > (4096|2048) \?", text["acm_kernels.hip"] + text["acm_parse.hip"])


def test_null_device_is_an_argument_error():
    caps, was = capi.LaunchCaps(list_slice=3), capi.LaunchCaps(dense_grid=7)
    assert capi.lib().acmhip_device_set_launch_caps(None, C.byref(caps), C.byref(was)) == capi.ERR_ARG
    assert capi.lib().acmhip_device_set_launch_caps(None, None, None) == capi.ERR_ARG
    assert was.as_dict() == dict(dict.fromkeys(FIELDS, 0), dense_grid=7)      # nothing written
    assert capi.lib().acmk_launch_caps_set(None, C.byref(caps), None) == capi.ERR_ARG


@pytest.mark.parametrize("field", FIELDS)
def test_a_cap_can_only_be_lowered(field):
    L = capi.lib()
    builtin = capi.LAUNCH_CAPS_BUILTIN[field]
    held = capi.LaunchCaps(**{f: 2 + k for k, f in enumerate(FIELDS)})
    before = held.as_dict()
    for bad in (builtin + 1, 0xFFFFFFFF):
        was = capi.LaunchCaps(**dict.fromkeys(FIELDS, 99))
        caps = capi.LaunchCaps(**{f: 1 for f in FIELDS})
        setattr(caps, field, bad)
        assert L.acmk_launch_caps_set(C.byref(held), C.byref(caps), C.byref(was)) == capi.ERR_ARG
        assert held.as_dict() == before and was.as_dict() == dict.fromkeys(FIELDS, 99)       # nothing changed, nothing reported
    for good in (1, builtin - 1, builtin, 0):
        caps = capi.LaunchCaps(**{field: good})
        assert L.acmk_launch_caps_set(C.byref(held), C.byref(caps), None) == 0
        assert held.as_dict() == dict(dict.fromkeys(FIELDS, 0), **{field: good})
        held = capi.LaunchCaps(**before)


def test_previous_round_trip():
    L = capi.lib()
    held = capi.LaunchCaps()
    first = capi.LaunchCaps(list_slice=3, small_grid_x=1, parse_slice=5, parse_grid_x=1, dense_grid=2)
    was = capi.LaunchCaps(**dict.fromkeys(FIELDS, 99))
    assert L.acmk_launch_caps_set(C.byref(held), C.byref(first), C.byref(was)) == 0
    assert was.as_dict() == dict.fromkeys(FIELDS, 0) and held.as_dict() == first.as_dict()      # a fresh handle: all built-in
    second = capi.LaunchCaps(dense_grid=1)
    was2 = capi.LaunchCaps()
    assert L.acmk_launch_caps_set(C.byref(held), C.byref(second), C.byref(was2)) == 0
    assert was2.as_dict() == first.as_dict() and held.as_dict() == dict(dict.fromkeys(FIELDS, 0), dense_grid=1)
    # NULL: the built-in values; previous may be the very struct that is handed in
    assert L.acmk_launch_caps_set(C.byref(held), None, C.byref(was)) == 0
    assert was.as_dict() == second.as_dict() and held.as_dict() == dict.fromkeys(FIELDS, 0)
    assert L.acmk_launch_caps_set(C.byref(held), C.byref(was2), C.byref(was2)) == 0
    assert held.as_dict() == first.as_dict() and was2.as_dict() == dict.fromkeys(FIELDS, 0)
    assert L.acmk_launch_caps_set(C.byref(held), C.byref(was2), None) == 0 and held.as_dict() == dict.fromkeys(FIELDS, 0)


@pytest.mark.gpu
def test_handles_keep_their_own_caps():
    """the caps live in the handle: a second handle keeps the built-in values, the context manager puts the previous ones back, and a
    refused call leaves the handle as it was"""
    import helpers  # noqa: F401  (fill mode, as in every GPU module)
    with capi.Device(0) as a, capi.Device(0) as b:
        with a.launch_caps(list_slice=3, dense_grid=2):
            assert b.set_launch_caps(None).as_dict() == dict.fromkeys(FIELDS, 0)
            with a.launch_caps(parse_slice=5):
                with pytest.raises(capi.AcmHipError):
                    a.set_launch_caps({"dense_grid": (1 << 20) + 1})
                assert a.set_launch_caps({"parse_slice": 5}).as_dict() == dict(dict.fromkeys(FIELDS, 0), parse_slice=5)
            assert a.set_launch_caps({"list_slice": 3, "dense_grid": 2}).as_dict() == dict(dict.fromkeys(FIELDS, 0), list_slice=3, dense_grid=2)
        assert a.set_launch_caps(None).as_dict() == dict.fromkeys(FIELDS, 0)
