#!/usr/bin/env python3
"""Generate tests/golden/reference_game.{npz,json} and reference_rows.{npz,json} by EXECUTING the reference's own game.py and collect.py (build container).

Pinned by running the reference's code, not a restatement of it:
  * ``Game.start_self_play`` (game.py:133-237) for ONE whole self-play game played by the reference's own ``MCTS_AI``
    (mcts.py) under ``np.random.seed``: the moves, pi of every ply, z, and the (aliased, game.py:234-237) history lists;
  * ``CollectPipeline.preprocess`` and ``flip_data`` (collect.py:64-131) applied to that game: the [17,7,10,9] float16 states
    incl. the constant turn plane (collect.py:78 reads a board that never advances), the mirrored states and pi[flip_map].
How: the modules import third-party packages that are absent here (cchess, h5py, IPython). Placeholder modules are registered
for them: ``h5py`` and ``IPython.display`` are never called on this path; ``cchess`` carries the names these modules touch
(``Board`` = the CPU oracle's duck-typed board, ``Move.from_uci / Move.uci``, ``RED``, ``BLACK``, an empty ``svg``), as
make_golden.py does for mcts.py. The evaluator is the deterministic hash evaluator of oracle/evaluators.py. So the vectors pin
the reference's game loop, temperature schedule, history bookkeeping, z assignment and tuple post-processing -- GIVEN the
oracle's rules (rules parity with cchess itself stays unpinned). Outputs are data only.

reference_rows.{npz,json} (``rows_main``): the per-ply histories of six such games -- ``Game.update_states_history`` (game.py:36-44) of the
running game object is wrapped and its red_states / black_states / board.turn are copied after every update, i.e. before game.py:234-237
aliases them away -- with pi, z, the moves, and the mirror pi of the reference's ``flip_data`` on the de-aliased tuples: what the DEFAULT
(per-sample history) mode of the product must write at every ply (tests/reference_rows.py).
"""
import json
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.environ.get("CCZ_GOLDEN_OUT", HERE)   # where the fixtures are written (tests/test_cpu_golden_regenerates.py: a scratch directory)
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from _ref_guard import assert_reference_untouched, silence_reference_log  # noqa: E402

from oracle import OracleBoard  # noqa: E402
from oracle.evaluators import hash_eval  # noqa: E402

REF = "/root/reference"
N_PLAYOUT, SALT, SCALE, SEED = 24, 17, 40.0, 321


def load_reference():
    ph = types.ModuleType("cchess")
    ph.RED, ph.BLACK = True, False
    ph.Board = OracleBoard

    class Move:
        @staticmethod
        def from_uci(s):
            return s

        @staticmethod
        def uci(m):
            return m

    ph.Move = Move
    ph.svg = types.ModuleType("cchess.svg")
    sys.modules["cchess"] = ph
    sys.modules["cchess.svg"] = ph.svg
    sys.modules["h5py"] = types.ModuleType("h5py")            # imported by collect.py, used only by collect_data's file I/O
    ipy, disp = types.ModuleType("IPython"), types.ModuleType("IPython.display")
    disp.display = lambda *a, **k: None
    disp.SVG = lambda *a, **k: None
    ipy.display = disp
    sys.modules["IPython"], sys.modules["IPython.display"] = ipy, disp
    sys.path.insert(0, REF)
    cwd = os.getcwd()
    os.chdir("/tmp")
    import collect as ref_collect  # noqa
    import game as ref_game  # noqa
    import mcts as ref_mcts  # noqa
    os.chdir(cwd)
    silence_reference_log(ref_collect, ref_game, ref_mcts)   # tools.log writes next to tools.py whatever the working directory is (tools.py:46-51)
    return ref_game, ref_mcts, ref_collect


# ---- reference_rows.{npz,json}: the per-ply histories the reference computes itself (update_states_history, game.py:36-44) and then
# aliases away (game.py:234-237), snapshotted while its own start_self_play runs. (n_playout, seed, salt): the first entry is the game of
# reference_game.npz; the others come from find_reference_games.py (scale 40, 8 playouts, salt 17 + seed % 5) and are hard-coded here.
ROW_GAMES = [(N_PLAYOUT, SEED, SALT), (8, 416, 18), (8, 417, 19), (8, 405, 17), (8, 421, 18), (8, 591, 18)]
ROW_FOURFOLD_SCAN = ("seeds 400..599 at 8 playouts (find_reference_games.py): 404 (647 plies), 540 (590), 562 (573) and 591 (543) end by fourfold "
                     "repetition; the shortest, 591, is the last game of the fixture")


def hash_policy(salt):
    def policy(board, red_states=None, black_states=None):
        ids = board.legal_ids()
        p, v = hash_eval(board.squares()[None, :], np.array([1 if board.turn else 0]), salt=salt, scale=SCALE)
        return zip(ids, p[0][ids]), np.array([[v[0]]], dtype=np.float32)
    return policy


def termination(board):
    """How the rules ended the game (the oracle's predicates, in the order game.py:208 / tools.py:109-123 ask them)."""
    if not board.legal_ids():
        return "checkmate" if board.in_check() else "stalemate"
    for name in ("insufficient_material", "fourfold_repetition", "sixty_moves"):
        if getattr(board, "is_" + name)():
            return name
    return "none"


def play_reference_game(ref_game, ref_mcts, n_playout, seed, salt):
    """One Game.start_self_play of the reference (its MCTS_AI, the hash evaluator, np.random.seed) with a snapshot of the game object's
    history lists and the side to move taken right after ITS update_states_history returns: after the update, before the push, so slot 0
    is the position the move is played in. Returns (game, play_data, moves, snapshots)."""
    player = ref_mcts.MCTS_AI(hash_policy(salt), c_puct=5, n_playout=n_playout, is_selfplay=True)
    moves, snaps = [], []
    orig_action = player.get_action

    def logged(board, temp=1e-3, return_prob=False, on_playout=None):
        r = orig_action(board, temp=temp, return_prob=return_prob, on_playout=on_playout)
        moves.append(int(r[0] if return_prob else r))
        return r

    player.get_action = logged
    game = ref_game.Game(OracleBoard())
    orig_update = game.update_states_history

    def snapshotting():
        orig_update()
        snaps.append((np.stack([np.asarray(s) for s in game.red_states]), np.stack([np.asarray(s) for s in game.black_states]),
                      bool(game.board.turn)))

    game.update_states_history = snapshotting
    np.random.seed(seed)
    play_data = game.start_self_play(player, is_shown=False, temp=1.0, game_index=7)
    assert len(play_data) == len(moves) == len(snaps)
    return game, play_data, moves, snaps


def rows_main(ref_game, ref_mcts, ref_collect):
    out, games = {}, []
    for g, (n_playout, seed, salt) in enumerate(ROW_GAMES):
        game, play_data, moves, snaps = play_reference_game(ref_game, ref_mcts, n_playout, seed, salt)
        T = len(play_data)
        hist = np.stack([np.concatenate((r, b), axis=0) for r, b, _ in snaps])
        assert hist.shape == (T, 16, 7, 10, 9) and np.isin(hist, (0, 1)).all()
        turn = np.array([1 if t else 0 for _, _, t in snaps], dtype=np.uint8)
        pi = np.stack([np.asarray(t[2], dtype=np.float64) for t in play_data])
        z = np.array([t[3] for t in play_data], dtype=np.float64)
        # the reference's own preprocess / flip_data (collect.py:64-131) on the DE-ALIASED tuples
        cp = ref_collect.CollectPipeline.__new__(ref_collect.CollectPipeline)
        cp.board = OracleBoard()
        processed = cp.preprocess([(list(r), list(b), pi[t], z[t]) for t, (r, b, _) in enumerate(snaps)])
        flipped = cp.flip_data(processed)
        assert len(processed) == T and len(flipped) == 2 * T
        pi_mirror = np.empty_like(pi)
        for t in range(T):
            st = np.asarray(processed[t][0])
            assert st.shape == (17, 7, 10, 9) and st.dtype == np.float16
            assert np.array_equal(st[:16], hist[t])                                  # planes 0-15 of processed row t ARE hist[t]
            assert np.array_equal(np.asarray(processed[t][1]), pi[t]) and processed[t][2] == z[t]
            fst = np.stack([np.asarray(p) for p in flipped[T + t][0]])
            assert np.array_equal(fst, st[..., ::-1])                                # every flipped plane: reversed along its last axis
            assert flipped[T + t][2] == z[t]                                         # flipped z == z
            pi_mirror[t] = np.asarray(flipped[T + t][1], dtype=np.float64)
        o = game.board.outcome() if game.board.is_game_over() else None
        winner = None if o is None or o.winner is None else bool(o.winner)
        assert np.array_equal(z, np.zeros(T) if winner is None else np.where(turn == (1 if winner else 0), 1.0, -1.0))
        out.update({f"g{g}_hist": hist.astype(np.int8), f"g{g}_turn": turn, f"g{g}_moves": np.array(moves, dtype=np.int32),
                    f"g{g}_pi": pi, f"g{g}_z": z, f"g{g}_pi_mirror": pi_mirror})
        games.append({"n_playout": n_playout, "seed": seed, "salt": salt, "scale": SCALE, "plies": T, "winner": winner,
                      "termination": termination(game.board)})
    meta = {"games": games,
            "arrays": "g<i>_hist int8 [T,16,7,10,9] (red slots 0-7, black slots 0-7; slot 0 = the position the move is played in), "
                      "g<i>_turn uint8 [T] (1 = red to move), g<i>_moves int32 [T], g<i>_pi float64 [T,2086], g<i>_z float64 [T], "
                      "g<i>_pi_mirror float64 [T,2086] (flip_data's pi)",
            "snapshot": "red_states / black_states / board.turn copied right after the game object's update_states_history returns "
                        "(after the update, before the push)",
            "turn_plane": "plane 16 of the reference's own rows is constant (collect.py:78 reads a board that never advances); the "
                          "default mode departs from that on purpose, so the expected plane 16 is the snapshotted turn, not collect.py's",
            "mirror": "asserted while generating: planes 0-15 of the reference's processed row t equal hist[t]; every plane flip_data "
                      "returns is the plane reversed along its last axis; flipped z equals z -- mirror states may be derived from hist",
            "fourfold_scan": ROW_FOURFOLD_SCAN}
    kinds = [(g["winner"], g["termination"], g["plies"]) for g in games]
    assert games[0]["plies"] == 72 and games[0]["winner"] is False
    assert any(w is True for w, _, _ in kinds) and sum(w is False for w, _, _ in kinds) >= 2
    assert any(w is None and term != "none" for w, term, _ in kinds) and any(p > 256 for _, _, p in kinds)
    assert kinds[-1][:2] == (None, "fourfold_repetition")
    np.savez_compressed(os.path.join(OUT, "reference_rows.npz"), **out)
    with open(os.path.join(OUT, "reference_rows.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(meta["games"])


def main():
    ref_game, ref_mcts, ref_collect = load_reference()

    def policy(board, red_states=None, black_states=None):
        ids = board.legal_ids()
        p, v = hash_eval(board.squares()[None, :], np.array([1 if board.turn else 0]), salt=SALT, scale=SCALE)
        return zip(ids, p[0][ids]), np.array([[v[0]]], dtype=np.float32)

    player = ref_mcts.MCTS_AI(policy, c_puct=5, n_playout=N_PLAYOUT, is_selfplay=True)
    moves = []
    orig = player.get_action

    def logged(board, temp=1e-3, return_prob=False, on_playout=None):
        r = orig(board, temp=temp, return_prob=return_prob, on_playout=on_playout)
        moves.append(int(r[0] if return_prob else r))
        return r

    player.get_action = logged
    np.random.seed(SEED)
    game = ref_game.Game(OracleBoard())
    play_data = game.start_self_play(player, is_shown=False, temp=1.0, game_index=7)
    T = len(play_data)
    assert T == len(moves)
    # the reference returns the SAME (final) history lists in every tuple (game.py:234-237)
    assert all(t[0] is play_data[0][0] and t[1] is play_data[0][1] for t in play_data)
    out = {"moves": np.array(moves, dtype=np.int32),
           "pi": np.stack([np.asarray(t[2], dtype=np.float64) for t in play_data]),
           "z": np.array([t[3] for t in play_data], dtype=np.float64),
           "final_red_states": np.stack([np.asarray(s) for s in play_data[0][0]]),
           "final_black_states": np.stack([np.asarray(s) for s in play_data[0][1]]),
           "final_sq": game.board.squares(), "final_turn": np.int32(1 if game.board.turn else 0)}
    meta = {"n_playout": N_PLAYOUT, "salt": SALT, "scale": SCALE, "seed": SEED, "plies": T,
            "pi_dtype": str(np.asarray(play_data[0][2]).dtype), "z_dtype": str(np.asarray(play_data[0][3]).dtype),
            "state_dtype": str(np.asarray(play_data[0][0][0]).dtype),
            "game_over": bool(game.board.is_game_over()), "tie": bool(game.board.is_tie()),
            "winner": None if game.board.outcome() is None or game.board.outcome().winner is None else bool(game.board.outcome().winner)}

    # ---- collect.py:64-131 on that game (no file I/O: the pipeline object is made without running its __init__)
    cp = ref_collect.CollectPipeline.__new__(ref_collect.CollectPipeline)
    cp.board = OracleBoard()           # collect.py:28: a board that is never advanced
    processed = cp.preprocess(play_data)
    assert len(processed) == T and cp.episode_len == T
    st = np.stack([np.asarray(p[0]) for p in processed])
    meta["processed_state_dtype"] = str(st.dtype)
    meta["processed_state_shape"] = list(st.shape)
    assert all(np.array_equal(st[0], s) for s in st)       # quirk: every sample carries the same (final) state
    out["processed_state"] = st[0]
    out["processed_pi"] = np.stack([np.asarray(p[1]) for p in processed])
    out["processed_z"] = np.array([p[2] for p in processed], dtype=np.float64)
    flipped = cp.flip_data(processed)
    assert len(flipped) == 2 * T
    fs = np.stack([np.asarray(p[0]) for p in flipped[T:]])
    assert all(np.array_equal(fs[0], s) for s in fs)
    out["flipped_state"] = np.asarray(fs[0])
    out["flipped_pi"] = np.stack([np.asarray(p[1]) for p in flipped[T:]])
    out["flipped_z"] = np.array([p[2] for p in flipped[T:]], dtype=np.float64)
    meta["flipped_state_dtype"] = str(fs.dtype)
    # ---- Game.start_play (game.py:77-130) between two non-self-play MCTS_AI players (mcts.py:225-229: temp 1e-3, tree
    # discarded after every move): the match path as the reference's own loop runs it
    def pol(salt):
        def f(board, red_states=None, black_states=None):
            ids = board.legal_ids()
            p, v = hash_eval(board.squares()[None, :], np.array([1 if board.turn else 0]), salt=salt, scale=SCALE)
            return zip(ids, p[0][ids]), np.array([[v[0]]], dtype=np.float32)
        return f

    red = ref_mcts.MCTS_AI(pol(31), c_puct=5, n_playout=30, is_selfplay=False)
    black = ref_mcts.MCTS_AI(pol(32), c_puct=5, n_playout=30, is_selfplay=False)
    match_moves = []
    for pl in (red, black):
        o = pl.get_action

        def lg(board, temp=1e-3, return_prob=False, on_playout=None, _o=o):
            r = _o(board, temp=temp, return_prob=return_prob, on_playout=on_playout)
            match_moves.append(int(r))
            return r
        pl.get_action = lg
    np.random.seed(SEED + 1)
    g2 = ref_game.Game(OracleBoard())
    winner = g2.start_play(red, black, is_shown=False)
    out["match_moves"] = np.array(match_moves, dtype=np.int32)
    out["match_final_sq"] = g2.board.squares()
    meta["match"] = {"salts": [31, 32], "n_playout": 30, "seed": SEED + 1, "plies": len(match_moves),
                     "winner": (-1 if winner == -1 else bool(winner)), "red_player_idx": red.player, "black_player_idx": black.player}

    np.savez_compressed(os.path.join(OUT, "reference_game.npz"), **out)
    with open(os.path.join(OUT, "reference_game.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(meta)
    rows_main(ref_game, ref_mcts, ref_collect)


if __name__ == "__main__":
    main()
    assert_reference_untouched()
