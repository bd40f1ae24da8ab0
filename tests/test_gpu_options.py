"""Every option of ``dmm_ctx_set_option`` reads back as ``opt_<name>``, and ``Context.options`` restores what it found.

On a ``Context`` of its own, not the shared ones: nothing here can leave an option set for another test.  No kernel
is launched."""

import os
import re

import pytest

pytestmark = pytest.mark.gpu

WORKSPACE = ["ml_workspace_mib", "regrid_workspace_mib", "wiener_workspace_mib"]
PLAIN = [
    "dirty_variant", "grid_mult", "dirty_static", "dirty_nofill", "dirty_prio", "project_variant", "project_grid_mult",
    "sht_variant", "sht_synth_form", "ringmap_variant", "ml_shortcut", "ml_eigen", "ml_null", "ml_reduce", "ml_rank_stop",
    "ml_chase_split", "ml_inner_sweeps", "ml_outer_sweeps", "gram_stage", "wiener_overlap",
]  # fmt: skip
OPTIONS = PLAIN + WORKSPACE + ["profile"]
DEFAULTS = {name: 0 for name in OPTIONS} | {"wiener_overlap": 1}


@pytest.fixture
def ctx():
    from draco_amd.device import Context

    return Context()


def test_the_list_is_the_documented_one():
    assert len(OPTIONS) == len(set(OPTIONS)) == 24
    header = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "include", "draco_amd.h")
    with open(header) as f:
        text = f.read()
    start = text.index("/* Options (name, integer value)")
    comment = text[start:text.index("*/", start)]
    rows = re.findall(r'^ \*   "(\w+)" +(-?\d+)  \S', comment, flags=re.M)
    assert len(rows) == 24 and {name for name, _ in rows} == set(OPTIONS)
    assert {name: int(default) for name, default in rows} == DEFAULTS


def test_defaults_on_a_fresh_context(ctx):
    assert {name: ctx.get_option(name) for name in OPTIONS} == DEFAULTS


def test_every_option_reads_back_what_was_set(ctx):
    for name in PLAIN:
        ctx.set_option(name, 3)
        assert ctx.get_option(name) == 3, name
        assert ctx.counter("opt_" + name) == 3 and ctx.get_option(name.encode()) == 3, name
    for name in WORKSPACE:
        ctx.set_option(name, -5)
        assert ctx.get_option(name) == 0, name
        ctx.set_option(name, 2048)
        assert ctx.get_option(name) == 2048, name
    ctx.set_option("profile", 1)
    assert ctx.get_option("profile") == 1
    ctx.set_option("profile", 0)
    assert ctx.get_option("profile") == 0
    # one row each: no option moved with another
    assert {name: ctx.get_option(name) for name in OPTIONS} == {name: 3 for name in PLAIN} | {name: 2048 for name in WORKSPACE} | {"profile": 0}


def test_scoped_options_restore_what_they_found(ctx):
    ctx.set_option("ml_shortcut", 3)
    with ctx.options(ml_shortcut=2, wiener_overlap=0):
        assert (ctx.get_option("ml_shortcut"), ctx.get_option("wiener_overlap")) == (2, 0)
    assert (ctx.get_option("ml_shortcut"), ctx.get_option("wiener_overlap")) == (3, 1)
    with pytest.raises(KeyError, match="from the body"):
        with ctx.options(ml_shortcut=2, wiener_overlap=0):
            assert (ctx.get_option("ml_shortcut"), ctx.get_option("wiener_overlap")) == (2, 0)
            raise KeyError("from the body")
    assert (ctx.get_option("ml_shortcut"), ctx.get_option("wiener_overlap")) == (3, 1)


def test_an_unknown_name_leaves_the_others_as_they_were(ctx):
    ctx.set_option("ml_shortcut", 3)
    with pytest.raises(ValueError, match="unknown option 'nope'"):
        with ctx.options(ml_shortcut=2, nope=1):
            raise AssertionError("the block must not be entered")
    assert ctx.get_option("ml_shortcut") == 3
    with pytest.raises(ValueError, match="unknown option 'nope'"):
        ctx.get_option("nope")
    with pytest.raises(ValueError, match="unknown option 'nope'"):
        ctx.set_option(b"nope", 1)
    with pytest.raises(ValueError, match="unknown counter 'nope'"):
        ctx.counter("nope")
