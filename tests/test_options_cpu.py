"""The option table of the library (csrc/options.hip) through lgd_set_option / lgd_get_option: defaults, allowed values,
refusals.  Host only."""
import os

import pytest

import lgd_amd  # noqa: F401
from lgd_amd import _lib

ERR_ARG = -1
# name: (default as include/lgd_hip.h documents it, allowed boundary values, values just outside, environment variable)
OPTIONS = {
    "cfg_pair": (1, (0, 1), (-1, 2), None),
    "gn_fused": (256, (0, 4096), (-1, 4097), None),
    "gn_slab": (1, (0, 1), (-1, 2), None),
    "ln_stream": (1, (0, 1), (-1, 2), None),
    "gn_apply_wgs": (1024, (64, 8192), (63, 8193, 0), None),
    "attn32": (1, (0, 2), (-1, 3), "LGD_ATTN32"),
    "attn32_nw": (8, (4, 8), (3, 5, 6, 9, 0), "LGD_ATTN32_NW"),
    "attn32_var": (0, (0, 2), (-1, 3), None),
    "attn_w4": (1, (0, 2), (-1, 3), "LGD_ATTN_W4"),
    "attn_w4_pipe": (1, (0, 1), (-1, 2), "LGD_W4_PIPE"),
}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


@pytest.mark.parametrize("name", list(OPTIONS))
def test_default_round_trip_and_refusal(lib, name):
    default, allowed, outside, env = OPTIONS[name]
    key = name.encode()
    before = lib.lgd_get_option(key)
    assert before >= 0
    # the documented default, unless this process was started with the option's variable or an LGD_OPTIONS entry for it
    if not (env and env in os.environ) and name not in os.environ.get("LGD_OPTIONS", ""):
        assert before == default
    try:
        for v in allowed:
            assert lib.lgd_set_option(key, v) == 0, v
            assert lib.lgd_get_option(key) == v
        kept = lib.lgd_get_option(key)
        for v in outside:
            assert lib.lgd_set_option(key, v) == ERR_ARG, v
            assert lib.lgd_get_option(key) == kept, v
    finally:
        assert lib.lgd_set_option(key, before) == 0
    assert lib.lgd_get_option(key) == before


def test_the_table_is_the_ten_options(lib):
    assert len(OPTIONS) == 10
    for name in ("attn_nw", "attn160", "attn_bwd", "LGD_ATTN_NW", "", "cfg_pair ", "CFG_PAIR"):    # environment-only switches stay unknown
        assert lib.lgd_get_option(name.encode()) == ERR_ARG, name
        assert lib.lgd_set_option(name.encode(), 1) == ERR_ARG, name
    assert lib.lgd_get_option(None) == ERR_ARG
    assert lib.lgd_set_option(None, 1) == ERR_ARG
