"""CPU: ``InferenceNet.tower_schedule``, the tower's launch structure as data, against literal schedules. Every measured decision about
the tower is in it -- two chains by default, three around 1024 boards, three with edge tiles from 4096, sequential groups above 4096,
one chain under stream capture -- and a wrong one is slower but still correct, so no value test sees it. The literals were worked out from
the formulas of the two launch loops this method replaced (the GPU twin, test_gpu_tower_launch_trace.py, compares the launches themselves
with a recording of those loops)."""
import pytest
import torch  # noqa: F401

G16, EDGE, ONE, QUAD = 64, 128, 512, 1 << 16      # CCZ_CONV_* flag bits (include/cczero.h)


@pytest.fixture(scope="module")
def inf():
    from chinesechesszero_amd.net import InferenceNet, Net
    return InferenceNet(Net(256, 1))


@pytest.fixture(autouse=True)
def default_options(inf):
    from chinesechesszero_amd.net import EvalOptions
    d = EvalOptions(env={})
    inf.set_options(**{f: getattr(d, f) for f in EvalOptions.FIELDS})


# padded boards, g16, edge tiles, dense ranges group by group, planned groups x chains, planned cap pixels
TABLE = [
    (8, False, False, [[(0, 8)]], (1, 1), 720),
    (600, False, False, [[(0, 384), (384, 600)]], (1, 2), 27360),
    (640, True, False, [[(0, 384), (384, 640)]], (1, 2), 28800),
    (656, True, False, [[(0, 384), (384, 656)]], (1, 2), 30240),          # 650 boards padded to whole groups of 16
    (1024, True, False, [[(0, 384), (384, 768), (768, 1024)]], (1, 3), 31680),
    (4096, True, True, [[(0, 1408), (1408, 2816), (2816, 4096)]], (1, 3), 123840),
    (4352, True, True, [[(0, 768), (768, 1536), (1536, 2176)], [(2176, 2944), (2944, 3712), (3712, 4352)]], (2, 3), 66240),
]


def flags(g16, edge):
    f2 = 1 | ((G16 | ((EDGE | ONE | QUAD) if edge else 0)) if g16 else 0)
    return f2 | 2, f2


@pytest.mark.parametrize("B,g16,edge,dense,shape,cap", TABLE, ids=[str(t[0]) for t in TABLE])
def test_schedules_under_default_options(inf, B, g16, edge, dense, shape, cap):
    assert inf._g16(B) == g16 and inf._edge(B, g16) == edge
    f1, f2 = flags(g16, edge)
    assert inf.tower_schedule(B, g16, False, False) == [[(lo, hi, f1, f2) for lo, hi in group] for group in dense]
    groups, chains = shape
    n_parts = groups * chains
    # part runs 0 .. n_parts - 1 in group-major order
    assert inf.tower_schedule(B, g16, True, False) == [[(cap, g * chains + k, n_parts, f1, f2) for k in range(chains)] for g in range(groups)]
    # under a stream capture: one group of one chain
    assert inf.tower_schedule(B, g16, False, True) == [[(0, B, f1, f2)]]
    one_cap = B // 16 * 1440 if g16 else -(-B // 8) * 8 * 90
    assert inf.tower_schedule(B, g16, True, True) == [[(one_cap, 0, 1, f1, f2)]]


def words(sched):
    return {d[-2:] for group in sched for d in group}


def test_flag_words_follow_the_options(inf):
    for planned in (False, True):
        assert words(inf.tower_schedule(600, False, planned)) == {(3, 1)}
        assert words(inf.tower_schedule(1024, True, planned)) == {(1 | 2 | G16, 1 | G16)}
        assert words(inf.tower_schedule(4096, True, planned)) == {(1 | 2 | G16 | EDGE | ONE | QUAD, 1 | G16 | EDGE | ONE | QUAD)}
    inf.set_options(zigzag=False)
    for planned in (False, True):
        assert words(inf.tower_schedule(600, False, planned)) == {(1, 1)}
        assert words(inf.tower_schedule(4096, True, planned)) == {(1 | G16 | EDGE | ONE | QUAD,) * 2}
    inf.set_options(zigzag=True, force="tile")       # force: the whole-batch form only (and no group-of-16 rows: _g16 is False)
    assert not inf._g16(1024)
    assert words(inf.tower_schedule(1024, False, False)) == {(1 | 2 | 32, 1 | 32)}
    assert words(inf.tower_schedule(1024, False, True)) == {(3, 1)}
    inf.set_options(force="", edge_tiles=False)
    for planned in (False, True):
        sched = inf.tower_schedule(4096, True, planned)
        assert words(sched) == {(1 | 2 | G16, 1 | G16)} and [len(g) for g in sched] == [2]      # no edge tiles: two chains
    inf.set_options(edge_tiles="auto", one_launch=False)
    for planned in (False, True):
        assert words(inf.tower_schedule(4096, True, planned)) == {(1 | 2 | G16 | EDGE | QUAD, 1 | G16 | EDGE | QUAD)}
    inf.set_options(one_launch=True, quad=False)
    for planned in (False, True):
        assert words(inf.tower_schedule(4096, True, planned)) == {(1 | 2 | G16 | EDGE | ONE, 1 | G16 | EDGE | ONE)}


def test_schedule_holds_plain_integers_and_the_library_constants(inf):
    from chinesechesszero_amd import _lib
    assert (G16, EDGE, ONE, QUAD) == (_lib.CONV_G16, _lib.CONV_G16_EDGE_TILES, _lib.CONV_G16_ONE_LAUNCH, _lib.CONV_G16_QUAD)
    for planned in (False, True):
        for group in inf.tower_schedule(4352, True, planned):
            assert all(type(v) is int for d in group for v in d)
