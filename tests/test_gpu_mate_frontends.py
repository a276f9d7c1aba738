"""GPU: the mate search in the front ends -- ``analyse --mate-search``, ``MCTS_AI(mate_search=...)``, the UCI loop's ``MateSearch`` option
and ``go mate N``, ``BatchedMatch`` and ``Arena`` -- on the fixtures of tests/mate_cases.py, with the expected moves and distances taken
from the sequential model (tests/mate_model.py).

The three-ply fixture of the one-game front ends is a mate by checks (``h10_dist3`` and its like), not ``mate_in_two`` of
tests/solver_cases.py: that position's three-ply win begins with a quiet move (i7i8), which a checking-sequence search does not look at
by definition (tests/test_cpu_mate_model.py shows it on the model and on the exhaustive negamax). ``mate_in_two`` is here as the
position on which the mate search finds nothing and the normal search answers."""
import functools
import io
import json

import numpy as np
import pytest
import torch

import mate_cases as mc
import mate_model as mm
from gpu_harness import planes_to_squares

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURES = mc.load()
NAMES = [f["name"] for f in FIXTURES]
SALT = 9


@functools.lru_cache(maxsize=None)
def model(name, plies=7, budget=2048):
    return mm.mate_search(mc.board(FIXTURES[NAMES.index(name)]), plies, budget)


def _fx(name):
    return FIXTURES[NAMES.index(name)]


def _mates(min_dist=1, turn=None, history=None):
    return [fx for fx in FIXTURES if model(fx["name"])[0] == mm.FOUND and model(fx["name"])[1] >= min_dist
            and (turn is None or fx["turn"] == turn) and (history is None or bool(fx["history"]) == history)]


def _hash_dense(leaf):
    from oracle.evaluators import hash_eval
    sq, turn = planes_to_squares(leaf.float().cpu().numpy())
    p, v = hash_eval(sq, np.asarray(turn).astype(np.int64), salt=SALT, scale=40.0)
    return torch.from_numpy(np.ascontiguousarray(p, np.float32)).to(leaf.device), torch.from_numpy(np.ascontiguousarray(v, np.float32).reshape(-1)).to(leaf.device)


def _fen(sq, turn, halfmove=0):
    from chinesechesszero_amd.game import _SYMBOL_INV
    rows = []
    for r in range(9, -1, -1):
        row, gap = "", 0
        for f in range(9):
            pc = int(sq[f + 9 * r])
            if not pc:
                gap += 1
                continue
            row += (str(gap) if gap else "") + (_SYMBOL_INV[pc & 7].upper() if pc < 8 else _SYMBOL_INV[pc & 7])
            gap = 0
        rows.append(row + (str(gap) if gap else ""))
    return "/".join(rows) + (" w" if turn else " b") + f" - - {halfmove} 1"


def _position(fx):
    return f"fen {_fen(mc.squares(fx), fx['turn'], fx['halfmove'])}" + (" moves " + " ".join(fx["history"]) if fx["history"] else "")


SIX = ("two_rooks", "h10_dist3", "h17_dist5", "h18_dist7", "mate_in_two", "h22_history")


def _load(e, fixtures):
    """The fixtures on the first boards of an engine (the rest parked); returns the sides to move."""
    B = e.B
    sq, turn, half, moves = np.zeros((B, 90), np.uint8), np.ones(B, np.uint8), np.zeros(B, np.int32), [[] for _ in range(B)]
    for b, fx in enumerate(fixtures):
        sq[b], turn[b], half[b], moves[b] = mc.squares(fx), fx["turn"], fx["halfmove"], [mc.move_id(u) for u in fx["history"]]
    assert not e.set_positions(sq, turn, half, moves, park=np.arange(B) >= len(fixtures)).any()
    return e.game_status()["turn"].astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- analyse
def _analyse(mate_search, solver=False, names=SIX):
    from chinesechesszero_amd.analyse import BatchedAnalysis
    an = BatchedAnalysis(_hash_dense, len(names), n_playout=24, seed=5, solver=solver, mate_search=mate_search, eval_cache_log2=0)
    return an, an.analyse([_position(_fx(n)) for n in names])


@pytest.mark.parametrize("solver", [False, True])
def test_analyse_names_the_mate_and_its_first_move(solver):
    an, recs = _analyse(7, solver)
    _, plain = _analyse(None, solver)
    assert {model(n)[0] for n in SIX} == {mm.FOUND, mm.NO_MATE}
    for name, rec, off in zip(SIX, recs, plain):
        st, dist, mv, _ = model(name)
        assert rec["status"] == "ok" and rec["lines"] == off["lines"] and rec["root_visits"] == off["root_visits"], name
        if st == mm.FOUND and not (solver and off.get("mate") is not None and 0 < off["mate"] <= (dist + 1) // 2):
            assert (rec["bestmove"], rec["mate"]) == (mc.uci(mv), (dist + 1) // 2), (name, rec["bestmove"], rec["mate"])
        else:
            assert (rec["bestmove"], rec["mate"]) == (off["bestmove"], off.get("mate")), name
    assert any(r["bestmove"] != o["bestmove"] for r, o in zip(recs, plain)) or solver
    s = an.summary()["mate_search"]
    assert (s["boards"], s["mates"]) == (len(SIX), sum(model(n)[0] == mm.FOUND for n in SIX)) and s["max_plies"] == 7
    assert s["mean_nodes"] == sum(model(n)[3] for n in SIX) / len(SIX)


def test_analyse_without_the_option_is_the_analysis_it_was():
    _, a = _analyse(None)
    _, b = _analyse(None)
    assert a == b and all("mate" not in r for r in a)
    an, _ = _analyse(None)
    assert "mate_search" not in an.summary()


def test_the_analyse_command_line(tmp_path):
    from chinesechesszero_amd import analyse
    src, out = tmp_path / "positions.txt", tmp_path / "out.jsonl"
    names = ("two_rooks", "h10_dist3", "mate_in_two")
    src.write_text("\n".join(_position(_fx(n)) for n in names) + "\n")
    torch.manual_seed(1)
    assert analyse.main([str(src), "--playout", "8", "--channels", "32", "--blocks", "1", "--out", str(out), "--mate-search", "7", "--mate-nodes", "512"]) == 0
    recs = [json.loads(l) for l in out.read_text().splitlines()]
    for name, rec in zip(names, recs):
        st, dist, mv, _ = model(name, 7, 512)
        if st == mm.FOUND:
            assert (rec["bestmove"], rec["mate"]) == (mc.uci(mv), (dist + 1) // 2), name
        else:
            assert rec["mate"] is None and rec["bestmove"] == rec["lines"][0]["moves"][0]
    with pytest.raises(SystemExit):
        analyse.main([str(src), "--mate-search", "6"])
    with pytest.raises(SystemExit):
        analyse.main([str(src), "--mate-nodes", "64"])


# ---------------------------------------------------------------------------------------------------------------- one game
class _CountingPolicy:
    """The hash evaluator in the reference's form ``f(board) -> (zip(ids, P[ids]), value)``, counting its calls."""
    def __init__(self):
        self.calls = 0

    def __call__(self, board, red_states=None, black_states=None):
        from oracle.evaluators import hash_eval
        self.calls += 1
        ids = board.legal_ids()
        p, v = hash_eval(board.squares()[None, :], np.array([1 if board.turn else 0]), salt=SALT, scale=1.0)
        return zip(ids, p[0][ids]), np.array([[v[0]]], dtype=np.float32)


def _board(fx):
    from chinesechesszero_amd.game import Board, Move
    b = Board(mc.squares(fx), bool(fx["turn"]), fx["halfmove"])
    for u in fx["history"]:
        b.push(Move.from_uci(u))
    return b


def test_mcts_ai_plays_the_mate_without_an_evaluator_call():
    from chinesechesszero_amd.mcts import MCTS_AI
    for name in ("h10_dist3", "h18_dist7"):
        st, dist, mv, nodes = model(name)
        policy = _CountingPolicy()
        ai = MCTS_AI(policy, c_puct=5, n_playout=16, mate_search={"plies": 7})
        move, probs = ai.get_action(_board(_fx(name)), return_prob=True)
        assert st == mm.FOUND and int(move) == mv and policy.calls == 0 and ai.last_mate == (mv, dist, nodes), name
        assert probs[mv] == 1.0 and probs.sum() == 1.0
        assert ai.mcts.options.mate_counts == {"boards": 1, "mates": 1, "nodes": nodes}
    # nothing found: the playouts run and the evaluator is asked (mate_in_two's win begins with a quiet move; h22's is blocked by its history)
    for name in ("mate_in_two", "h22_history"):
        policy = _CountingPolicy()
        ai = MCTS_AI(policy, c_puct=5, n_playout=16, mate_search=7)
        move = ai.get_action(_board(_fx(name)))
        assert model(name)[0] == mm.NO_MATE and ai.last_mate is None and policy.calls > 0 and int(move) in mc.board(_fx(name)).legal_ids()
    # off: no query is made at all
    policy = _CountingPolicy()
    ai = MCTS_AI(policy, c_puct=5, n_playout=16)
    ai.get_action(_board(_fx("h10_dist3")))
    assert ai.last_mate is None and policy.calls > 0 and ai.mcts.options.mate_counts == {"boards": 0, "mates": 0, "nodes": 0}


def _uci(lines):
    from chinesechesszero_amd.uci import UciLoop
    out = io.StringIO()
    policy = _CountingPolicy()
    loop = UciLoop(policy_value_fn=policy, n_playout=16, out=out)
    for line in lines:
        assert loop.handle(line)
    return out.getvalue().splitlines(), policy


def test_uci_go_mate_and_the_matesearch_option():
    st, dist, mv, nodes = model("h10_dist3")
    assert (st, dist) == (mm.FOUND, 3)
    text, policy = _uci([f"position {_position(_fx('h10_dist3'))}", "go mate 2"])
    assert f"info depth 3 score mate 2 nodes {nodes} pv {mc.uci(mv)}" in text and text[-1] == f"bestmove {mc.uci(mv)}" and policy.calls == 0
    text, policy = _uci([f"position {_position(_fx('h10_dist3'))}", "go mate 1"])           # one ply is not enough: the normal search answers
    assert not any("score mate" in l for l in text) and text[-1].startswith("bestmove ") and policy.calls > 0
    for name in ("mate_in_two", "h05_nomate"):                                                 # state 2: falls back to a normal bestmove
        assert model(name, 3)[0] == mm.NO_MATE
        text, policy = _uci([f"position {_position(_fx(name))}", "go mate 2"])
        best = [l for l in text if l.startswith("bestmove ")]
        assert len(best) == 1 and any(" score cp " in l for l in text) and not any("score mate" in l for l in text) and policy.calls > 0
        assert mc.move_id(best[0].split()[1]) in mc.board(_fx(name)).legal_ids()
    st7 = model("h18_dist7")
    text, policy = _uci(["setoption name MateSearch value 7", f"position {_position(_fx('h18_dist7'))}", "go"])
    assert f"info depth 7 score mate 4 nodes {st7[3]} pv {mc.uci(st7[2])}" in text and text[-1] == f"bestmove {mc.uci(st7[2])}" and policy.calls == 0
    text, policy = _uci([f"position {_position(_fx('h18_dist7'))}", "go"])                    # MateSearch 0: as ever
    assert not any("score mate" in l for l in text) and policy.calls > 0


# ---------------------------------------------------------------------------------------------------------------- lockstep matches
def _oracle_argmax(fx, n_playout):
    """The most visited move of the sequential reference search under the hash evaluator (oracle.OracleMCTS)."""
    from oracle import OracleMCTS
    from oracle.evaluators import hash_eval

    def ev(board, ids):
        p, v = hash_eval(board.squares()[None, :], np.array([1 if board.turn else 0]), salt=SALT, scale=40.0)
        return p[0][ids], v[0]
    acts, visits, _ = OracleMCTS(ev, c_puct=5, n_playout=n_playout).get_move_probs(mc.board(fx))
    return int(acts[int(np.argmax(visits))])


def test_batched_match_plays_the_mating_move():
    from chinesechesszero_amd.match import BatchedMatch
    red = _mates(min_dist=3, turn=1)
    away = [fx["name"] for fx in red if _oracle_argmax(fx, 24) != model(fx["name"])[2]]
    assert away, "no fixture on which the most visited move is another one"
    played = {}
    for on in (None, {"plies": 7, "nodes": 2048}):
        m = BatchedMatch(_hash_dense, _hash_dense, len(red) + 1, n_playout=24, seed=2, mate_search=on)
        _load(m.engine, red)
        played[on is not None] = m.play_move(1)
        if on:
            assert m.options.report(m.engine)["mate_search"]["mates"] == len(red) and m.options.mate_counts["boards"] == len(red)
    for b, fx in enumerate(red):
        assert played[True][b] == model(fx["name"])[2], fx["name"]
    assert any(played[False][b] != model(fx["name"])[2] for b, fx in enumerate(red) if fx["name"] in away)
    assert played[True][len(red)] == -1


def test_arena_plays_the_mating_move():
    from test_gpu_arena import _logits_evaluators
    from chinesechesszero_amd.arena import Arena
    some = _mates(min_dist=3, history=False)[:8]
    assert len(some) == 8 and {fx["turn"] for fx in some} == {0, 1}
    ev = _logits_evaluators([3, 3])
    played = {}
    for on in (None, 7):
        ar = Arena(ev[0], ev[1], 4, n_playout=16, opening_plies=2, seed=4, eval_cache_log2=12, mate_search=on)
        ar._turn = _load(ar.engine, some)
        played[on is not None] = ar.play_move()
        if on:
            assert ar.result()["mate_search"]["mates"] == 8
    want = [model(fx["name"])[2] for fx in some]
    assert list(played[True]) == want and list(played[False]) != want
