"""full_sequence's four map stages (world_map_prune, world_map_components, world_map_outliers, world_map_shapes): every
refusal of their options with its exact text, and which refusal wins when two keywords are wrong at once.  The options are
checked before anything touches a device, so a stand-in object serves as the map."""
import inspect

import pytest

from dvs_mcemvs_amd import process as proc

MAP = object()
GOOD = {"world_map_prune": {}, "world_map_components": {}, "world_map_outliers": {"k": 4, "radius": 0.1},
        "world_map_shapes": {"k": 4, "radius": 0.1}}
NEEDS_K = {"world_map_outliers", "world_map_shapes"}
NEEDS_CLOUD = "world_map needs options_depth_map and options_point_cloud: the map is made of the windows' clouds"


def refusal(**kw):
    with pytest.raises(ValueError) as e:
        next(proc.full_sequence(None, None, None, None, None, 0.0, 1.0, 0.1, 1, **kw))
    return str(e.value)


def test_the_four_keywords_are_explicit_and_off_by_default():
    params = inspect.signature(proc.full_sequence).parameters
    for name in GOOD:
        assert params[name].default is None and params[name].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD, name
        assert name + "=" in proc.full_sequence.__doc__


@pytest.mark.parametrize("name", sorted(GOOD))
def test_every_refusal_has_its_text(name):
    good = GOOD[name]
    assert refusal(**{name: good}) == "%s needs world_map" % name
    for every in (0, 1.5, -1):
        assert refusal(world_map=MAP, **{name: dict(good, every=every)}) == "%s['every'] must be an integer >= 1" % name
    assert refusal(world_map=MAP, **{name: dict(good, zeta=1, alpha=2)}) == "%s: unknown keys ['alpha', 'zeta']" % name
    if name in NEEDS_K:
        for missing in ("k", "radius"):
            assert refusal(world_map=MAP, **{name: {k: v for k, v in good.items() if k != missing}}) == "%s needs k and radius" % name
        assert refusal(world_map=MAP, **{name: {}}) == "%s needs k and radius" % name
    # accepted options reach the checks that follow the four stages
    assert refusal(world_map=MAP, **{name: dict(good, every=3)}) == NEEDS_CLOUD
    assert refusal(world_map=MAP, **{name: dict(good, every=2.0)}) == NEEDS_CLOUD


def test_refusals_of_one_stage_alone():
    keep = "world_map_shapes['keep'] must name at least one of linear, planar and scattered"
    assert refusal(world_map=MAP, world_map_shapes={"k": 4, "radius": 0.1, "keep": ()}) == keep
    assert refusal(world_map=MAP, world_map_shapes={"k": 4, "radius": 0.1, "keep": 0}) == keep
    assert refusal(world_map=MAP, world_map_shapes={"k": 4, "radius": 0.1, "keep": 8}) == keep
    assert refusal(world_map=MAP, world_map_shapes={"k": 4, "radius": 0.1, "keep": ("flat",)}) == \
        "unknown shape 'flat': linear, planar or scattered"
    both = "world_map_prune takes box or local_box, not both"
    box = ((0, 0, 0), (1, 1, 1))
    assert refusal(world_map=MAP, world_map_prune={"box": box, "local_box": (1, 1, 1)}) == both
    assert refusal(world_map=MAP, world_map_prune={"box": None, "local_box": (1, 1, 1)}) == NEEDS_CLOUD
    assert refusal(world_map=MAP, world_map_prune={"box": box, "max_age": 3, "every": 2}) == NEEDS_CLOUD
    # the order inside one stage: every, the box, unknown keys; every, unknown keys, k and radius, keep
    assert refusal(world_map=MAP, world_map_prune={"box": box, "local_box": (1, 1, 1), "every": 0}) == \
        "world_map_prune['every'] must be an integer >= 1"
    assert refusal(world_map=MAP, world_map_prune={"box": box, "local_box": (1, 1, 1), "zeta": 1}) == both
    assert refusal(world_map=MAP, world_map_shapes={"radius": 0.1, "zeta": 1}) == "world_map_shapes: unknown keys ['zeta']"
    assert refusal(world_map=MAP, world_map_shapes={"radius": 0.1, "keep": ()}) == "world_map_shapes needs k and radius"
    # every stage accepts all the keywords of its two calls
    full = {"world_map_prune": dict(min_points=1, min_windows=1, max_age=2, box=box, reach=1, min_neighbors=1, shrink=True),
            "world_map_components": dict(min_points=1, min_windows=1, connectivity=6, min_cells=2, min_component_points=2,
                                         keep_largest=1, shrink=True),
            "world_map_outliers": dict(k=4, radius=0.1, min_found=1, min_points=1, min_windows=1, std_mult=1.0, shrink=True),
            "world_map_shapes": dict(k=4, radius=0.1, min_found=2, orient=True, viewpoint=(0, 0, 0), min_points=1, min_windows=1,
                                     keep=("planar",), remove_sparse=False, shrink=True)}
    assert refusal(world_map=MAP, **full) == NEEDS_CLOUD
    # a key of another stage, or of the dry runs' fetches, is unknown
    assert refusal(world_map=MAP, world_map_outliers={"k": 4, "radius": 0.1, "keep": ("planar",)}) == \
        "world_map_outliers: unknown keys ['keep']"
    assert refusal(world_map=MAP, world_map_components={"local_box": (1, 1, 1)}) == "world_map_components: unknown keys ['local_box']"


def test_which_refusal_wins():
    """today's order: shapes, outliers, components, prune, then the checks of world_map itself"""
    order = ["world_map_shapes", "world_map_outliers", "world_map_components", "world_map_prune"]
    for first, second in zip(order, order[1:]):
        # one error kind each, so that the text tells the stage and the kind
        kw = {first: dict(GOOD[first], every=0), second: dict(GOOD[second], zeta=1)}
        assert refusal(world_map=MAP, **kw) == "%s['every'] must be an integer >= 1" % first
        kw = {first: dict(GOOD[first], zeta=1), second: dict(GOOD[second], every=0)}
        assert refusal(world_map=MAP, **kw) == "%s: unknown keys ['zeta']" % first
        assert refusal(**{first: GOOD[first], second: GOOD[second]}) == "%s needs world_map" % first
    assert refusal(world_map=MAP, world_map_prune={"every": 0}) == "world_map_prune['every'] must be an integer >= 1"
    assert refusal(world_map=MAP, concurrent=True, world_map_prune={"zeta": 1}) == "world_map_prune: unknown keys ['zeta']"
    all_wrong = {name: dict(GOOD[name], every=0) for name in order}
    assert refusal(world_map=MAP, **all_wrong) == "world_map_shapes['every'] must be an integer >= 1"
    assert refusal(world_map=MAP, options_point_cloud=object(), concurrent=True) == \
        "world_map lives on one context: concurrent=True gives every window in flight its own"
