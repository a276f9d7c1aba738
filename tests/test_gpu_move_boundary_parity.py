"""GPU: the two ways onto a root position agree under CCZ_RULE_PERPETUAL_CHECK -- a history loaded in one launch (ccz_set_positions:
the replay loop keeps the chain's in-check bits and restarts them on a zeroing move) and the same moves played one by one
(ccz_finish_move, forced). The perpetual-check tests of test_gpu_rule_tables.py play through finish_move and the loading tests of
test_gpu_analysis.py run with the rule off, so nothing else reads the bits the loader writes. No search: every move is forced."""
import contextlib

import numpy as np
import pytest

from golden_cases import _place, perpetual_case, perpetual_quiet_cycle

pytestmark = pytest.mark.gpu

@contextlib.contextmanager
def _rules(flag):
    import oracle
    from chinesechesszero_amd import tools
    try:
        oracle.set_rules(perpetual_check=flag)
        tools.set_rules(perpetual_check=flag)
        yield
    finally:
        oracle.set_rules()
        tools.set_rules()


@pytest.fixture(scope="module")
def pair_of():
    """pair_of(flag): one engine pair (two boards each) per rule setting -- the rule is engine-wide and picked up at creation, so call it
    inside _rules(flag). The engines are closed when the module is done."""
    made = {}

    def get(flag):
        if flag not in made:
            from chinesechesszero_amd.engine import SelfPlayEngine
            made[flag] = tuple(SelfPlayEngine(2, n_playout=8, seed=3, strict=True) for _ in range(2))
            assert all(e.perpetual_check is flag for e in made[flag])
        return made[flag]
    yield get
    for pair in made.values():
        for e in pair:
            e.close()


def _snapshot(e):
    st = e.game_status()
    return {"squares": e.root_positions(), "turn": st["turn"].copy(), "over": st["over"] != 0, "winner": st["winner"].astype(int)}


def _same(x, y, what):
    for f in ("squares", "turn", "over", "winner"):
        assert np.array_equal(x[f], y[f]), (what, f, x[f], y[f])


def _run(pair_of, flag, lines):
    """lines: two (squares, turn, halfmove, [uci]) of equal length, one per board. Loads them at once, loads all but the last move and plays
    it, plays them one by one: the three engine states must be equal, and end the game as the oracle does. Returns the oracle's
    [(over, winner)]."""
    import oracle
    from oracle import OracleBoard
    ID = {u: i for i, u in enumerate(oracle.move_table())}
    sq = np.stack([l[0] for l in lines])
    turn, half = [l[1] for l in lines], [l[2] for l in lines]
    ids = np.array([[ID[u] for u in l[3]] for l in lines], np.int32)
    n = ids.shape[1]
    with _rules(flag):
        a, b = pair_of(flag)
        want = []
        for s, t, h, ucis in lines:
            ob = OracleBoard.from_array(s, t, h)
            for i, u in enumerate(ucis):
                assert ID[u] in ob.legal_ids() and not ob.is_game_over(), (u, i)   # the line is legal and alive up to its last move
                ob.push(u)
            w = ob.outcome().winner if ob.is_game_over() else None
            want.append((ob.is_game_over(), -1 if w is None else int(w)))
        # A: the whole line in one launch
        status = a.set_positions(sq, turn, half, [list(r) for r in ids])
        assert not status.any(), status
        full = _snapshot(a)
        # A again: all but the last move loaded -- the board is live --, the last one played: k_finish_move reads the loaded check bits
        status = a.set_positions(sq, turn, half, [list(r[:-1]) for r in ids])
        assert not status.any(), status
        assert not a.game_status()["over"].any()
        a.finish_move(forced_moves=ids[:, -1].copy(), keep_tree=False)
        last_played = _snapshot(a)
        # B: set_position and one forced finish_move per ply
        for j in range(2):
            b.set_position(j, sq[j], turn[j], half[j])
        for i in range(n):
            assert not b.game_status()["over"].any(), i
            b.finish_move(forced_moves=ids[:, i].copy(), keep_tree=False)
        played = _snapshot(b)
        a.check_healthy()
        b.check_healthy()
    _same(full, played, "loaded at once / played")
    _same(last_played, played, "last move played / played")
    for j, (over, winner) in enumerate(want):
        assert (bool(played["over"][j]), int(played["winner"][j])) == (over, winner), (j, played, want)
    return want


def _cycle_lines(cycle_of, halfmoves=(0, 0), colours=(True, False)):
    out = []
    for red, h in zip(colours, halfmoves):
        pos, turn, _ = perpetual_case(red)
        out.append((pos, turn, h, [cycle_of(red)[i % 4] for i in range(12)]))
    return out


@pytest.mark.parametrize("flag,quiet,winners", [(True, False, [0, 1]), (False, False, [-1, -1]), (True, True, [-1, -1])],
                         ids=["checking_cycle_rule_on", "checking_cycle_rule_off", "quiet_shuffle_rule_on"])
def test_loaded_history_and_played_history_end_the_game_alike(pair_of, flag, quiet, winners):
    """Three cycles of the rook-and-bare-king lines, red and black as the checker (board 0 / board 1): twelve moves loaded at once,
    eleven loaded and the twelfth played, twelve played. Root position, side to move, over and winner are equal between the three and
    equal to the oracle's: under the rule the side that checked with every move loses, otherwise the fourfold repetition is a draw."""
    lines = _cycle_lines(perpetual_quiet_cycle if quiet else (lambda red: perpetual_case(red)[2]))
    want = _run(pair_of, flag, lines)
    assert want == [(True, w) for w in winners]


def _window_verdict(bits, first_occ, turn):
    """The perpetual-check rule on a chain's in-check bits -- bits[i]: the side to move stands in check at chain
    position i, so the move that led there gave check; turn: the side to move at the last position. Inside the window after the
    repeated position's first occurrence, a side whose every move gave check while the other's did not loses. The winner, or -1."""
    last = len(bits) - 1
    window = range(first_occ + 1, last + 1)
    mover = [bits[i] for i in window if (last - i) % 2 == 0]      # the side that made the last move
    other = [bits[i] for i in window if (last - i) % 2 == 1]
    mover_all, other_all = all(mover), bool(other) and all(other)
    return turn if mover_all and not other_all else turn ^ 1 if other_all and not mover_all else -1


def test_zeroing_move_restarts_the_check_bits_of_a_loaded_history(pair_of):
    """Two plies before the cycles: the rook checks and the checked king captures a pawn, arriving at the position of perpetual_case
    with the clock and the history chain restarted. The first cycle after the capture opens with a quiet rook move and only then
    checks; two checking cycles follow. Inside the repetition window the rook's side has not checked with every move, so the game is a
    draw under the rule. The quiet move's position has chain index 1 -- the index at which the check before the capture was marked: a
    loader (or a push) that kept that bit across the zeroing move would see a check with every move and make the checker lose."""
    from oracle import OracleBoard
    prefix = {True: (_place({"d0": 7, "a6": 3, "e9": 1, "e8": 7 + 8}), 1, ["a6a8", "e8e9"], ["a8a7", "e9e8", "a7a8", "e8e9"]),
              False: (_place({"d9": 7 + 8, "a3": 3 + 8, "e0": 1 + 8, "e1": 7}), 0, ["a3a1", "e1e0"], ["a1a2", "e0e1", "a2a1", "e1e0"])}
    lines = []
    for red in (True, False):
        pos, turn, pre, late_check = prefix[red]
        target, target_turn, cycle = perpetual_case(red)
        after = late_check + cycle + cycle
        lines.append((pos, turn, 40, pre + after))
        with _rules(True):   # the preconditions, on the CPU
            ob = OracleBoard.from_array(pos, turn, 40)
            ob.push(pre[0])
            assert ob.in_check() and ob.halfmove == 41          # chain index 1 of the old chain: a check
            ob.push(pre[1])
            assert ob.halfmove == 0 and np.array_equal(ob.squares(), target) and int(ob.turn) == target_turn
            checks = []
            for i, u in enumerate(after):
                assert not ob.is_fourfold_repetition(), i
                ob.push(u)
                checks.append(ob.in_check())
            assert ob.is_fourfold_repetition() and ob.halfmove == 12
            assert checks == [False, False] + [True, False] * 5  # chain index 1 of the new chain: no check; every later rook move checks
            bits = [False] + checks                              # the new chain: index 0 is the position the capture reached
            kept = [False, True] + checks[1:]                    # ... had the old chain's bit at index 1 survived the capture
            turn_end = int(ob.turn)
            assert _window_verdict(bits, 0, turn_end) == -1 and _window_verdict(kept, 0, turn_end) == (0 if red else 1)
            assert ob.outcome().winner is None
    want = _run(pair_of, True, lines)
    assert want == [(True, -1), (True, -1)]


def test_loaded_cycle_that_coincides_with_the_sixty_move_draw_is_a_draw(pair_of):
    """The clock case of test_gpu_rule_tables.py through the loader: red checks for three cycles; from clock 108 the repetition
    completes at the ply the clock reaches 120 and the game is a draw, from clock 100 the checker loses."""
    lines = _cycle_lines(lambda red: perpetual_case(red)[2], halfmoves=(108, 100), colours=(True, True))
    want = _run(pair_of, True, lines)
    assert want == [(True, -1), (True, 0)]
