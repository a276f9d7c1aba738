"""GPU: resignation in the checkpoint arena (chinesechesszero_amd/arena.py, ``Arena(resign=...)``). Eight pairs with stub
evaluators in the style of test_gpu_arena.py: a resigned game is a win for the other side and never a truncated one, the
``resigned`` count of the result is the engine's status count, and without the option the result is the dict it always was."""
import numpy as np
import pytest
import torch

from chinesechesszero_amd import _lib

pytestmark = pytest.mark.gpu

PAIRS, PLAYOUT, MAXP = 8, 16, 10
RESIGN = {"threshold": -0.9, "consecutive": 2, "min_ply": 0}


class ValueStub:
    """A plan-capable logits evaluator: uniform logits, value = -c where the leaf's turn plane says red is to move, +c otherwise --
    a pure function of the position, as the shared evaluation cache needs. With c = 0.95 every red root sits at -0.95."""
    batched = True
    returns_logits = True
    accepts_plan = True
    stateless = True

    def __init__(self, c):
        self.c = float(c)

    def __call__(self, leaf, plan=None):
        n = leaf.shape[0]
        if plan is not None:
            rows, _ = plan
            leaf = leaf.index_select(0, rows.long().clamp(0, n - 1))         # compact: row i = board rows[i]
        red = leaf[:, 16, 0, 0, 0] > 0
        value = torch.where(red, torch.full_like(red, -self.c, dtype=torch.float32), torch.full_like(red, self.c, dtype=torch.float32))
        return torch.zeros((n, 2086), dtype=torch.float32, device=leaf.device), value.contiguous()


def _arena(c_a, c_b, **kw):
    from chinesechesszero_amd.arena import Arena
    return Arena(ValueStub(c_a), ValueStub(c_b), PAIRS, n_playout=PLAYOUT, opening_plies=4, seed=2, max_plies=MAXP, eval_cache_log2=12, **kw)


def _plain(r):
    return {k: v for k, v in r.items() if k not in ("wall_s", "games_per_s")}


def test_resigned_games_are_wins_and_losses_never_truncated():
    """Both networks see red at -0.95: red resigns at its second move on every board; A plays red on the even boards."""
    ar = _arena(0.95, 0.95, resign=RESIGN)
    assert (ar.engine.game_status()["turn"] == 1).all()                      # 4-ply openings: red to move
    r = ar.play()
    st, rs = ar.engine.game_status(), ar.engine.resign_status()
    assert (rs["state"] == (_lib.RESIGN_RESIGNED | 1)).all() and (rs["fire_ply"] == 2).all()
    assert (st["winner"] == 0).all() and (st["plies"] == 3).all()
    assert r["resigned"] == int(((rs["state"] & _lib.RESIGN_RESIGNED) != 0).sum()) == 2 * PAIRS
    assert (r["wins"], r["draws"], r["losses"], r["truncated"], r["unfinished"]) == (PAIRS, 0, PAIRS, 0, 0)
    assert r["score"] == 0.5 and r["pentanomial"] == [0, 0, PAIRS, 0, 0] and not ar.truncated.any()
    assert all((m[:] >= 0).all() for m in ar.moves[:2]) and (ar.moves[2] == -1).all() and len(ar.moves) == 3
    assert ar.engine.resign_stats()["resigned_games"] == 2 * PAIRS and ar.engine.resign_stats()["playon_games"] == 0


def test_resigned_and_truncated_games_side_by_side():
    """A sees red at -0.95, B at -0.5: A resigns where it plays red (the even boards); the odd boards run into the ply cap."""
    ar = _arena(0.95, 0.5, resign=RESIGN)
    r = ar.play()
    rs = ar.engine.resign_status()
    even = np.arange(2 * PAIRS) % 2 == 0
    assert np.array_equal((rs["state"] & _lib.RESIGN_RESIGNED) != 0, even)
    assert np.array_equal(ar.truncated, ~even)
    assert (r["wins"], r["draws"], r["losses"], r["truncated"], r["resigned"], r["unfinished"]) == (0, PAIRS, PAIRS, PAIRS, PAIRS, 0)
    assert r["resigned"] == int(((rs["state"] & _lib.RESIGN_RESIGNED) != 0).sum())
    assert r["pentanomial"] == [0, PAIRS, 0, 0, 0]


def test_without_the_option_the_result_is_what_it_was():
    """resign=None: no ``resigned`` key, the engine never hears of the feature. And an arena whose rule can never fire (both
    networks at 0.5) plays the same games: its result is that dict plus ``resigned`` = 0."""
    plain = _arena(0.5, 0.5)

    def never(*a, **kw):
        raise AssertionError("the arena without resign= configured resignation")
    plain.engine.set_resign = never
    plain.engine.resign_status = never
    r0 = _plain(plain.play())
    assert "resigned" not in r0 and r0["truncated"] == 2 * PAIRS == r0["draws"]
    assert list(r0) == ["pairs", "games", "n_playout", "n_playout_b", "wins", "draws", "losses", "truncated", "unfinished", "pentanomial", "score",
                        "score_se", "score_ci95", "elo", "elo_ci95", "plies_mean", "plies_min", "plies_max", "steps", "rows_per_step", "cache"]
    calm = _arena(0.5, 0.5, resign=RESIGN)
    r1 = _plain(calm.play())
    assert r1.pop("resigned") == 0 and r1 == r0
    assert len(plain.moves) == len(calm.moves) and all(np.array_equal(x, y) for x, y in zip(plain.moves, calm.moves))


def test_the_arena_plays_no_game_on():
    with pytest.raises(ValueError, match="p_playon"):
        _arena(0.95, 0.95, resign={"threshold": -0.9, "p_playon": 0.5})
    ar = _arena(0.95, 0.95, resign=-0.9)                                     # a bare threshold: the engine's defaults, min_ply 30
    assert ar.resign == {"threshold": -0.9, "p_playon": 0.0}
    r = ar.play()
    assert r["resigned"] == 0 and r["truncated"] == 2 * PAIRS                # 10-ply games never reach ply 30
