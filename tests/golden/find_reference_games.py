"""How the games of reference_rows.npz were CHOSEN (build container only; make_golden_game.py hard-codes the result in ROW_GAMES):
a bounded scan of seeds, each one whole Game.start_self_play of the reference under the hash evaluator (scale 40, 8 playouts, salt
17 + seed % 5), listing plies, winner and how the rules ended the game. Wanted: a red win, two black wins, a draw by the rules, a game
longer than 256 plies, and -- if the scan turns one up -- a game that ends by fourfold repetition.

    python tests/golden/find_reference_games.py 400 600      # ~200 games of 1-4 s each, spread over the cores
"""
import os
import sys
from multiprocessing import Pool

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

N_PLAYOUT = 8


def one(seed):
    import make_golden_game as G
    ref_game, ref_mcts, _ = G.load_reference()
    game, play_data, _, _ = G.play_reference_game(ref_game, ref_mcts, N_PLAYOUT, seed, 17 + seed % 5)
    o = game.board.outcome() if game.board.is_game_over() else None
    winner = None if o is None or o.winner is None else bool(o.winner)
    return seed, len(play_data), winner, G.termination(game.board)


if __name__ == "__main__":
    lo, hi = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (400, 600)
    with Pool(min(16, os.cpu_count() or 1), maxtasksperchild=8) as pool:
        rows = sorted(pool.imap_unordered(one, range(lo, hi)))
    print("| seed | plies | winner | ended by |\n|---|---|---|---|")
    for seed, plies, winner, term in rows:
        print(f"| {seed} | {plies} | {'draw' if winner is None else ('red' if winner else 'black')} | {term} |")
    print("fourfold_repetition:", [r[0] for r in rows if r[3] == "fourfold_repetition"] or "none")
