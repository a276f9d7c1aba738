"""How tests/golden/mate_cases.json was found: the sequential model (tests/mate_model.py) over seeded random small-material positions,
kept where a category of tests/test_cpu_mate_model.py still had room. Run from the repository root:

    python tests/golden/make_mate_cases.py > tests/golden/mate_cases.json

The file holds placements, histories and the budgets to test at; every expected number is recomputed by the tests."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

import mate_cases as mc        # noqa: E402
import mate_model as mm        # noqa: E402
from golden_cases import STARTS, sq   # noqa: E402
from oracle import OracleBoard, lib   # noqa: E402

PLIES, BIG = 7, 16384
FILES = "abcdefghi"


def name_of(s):
    return FILES[s % 9] + str(s // 9)


def random_position(rs):
    """(squares, turn): kings, two to four attacking pieces of the side to move, up to four of the other side's."""
    turn = int(rs.randint(2))
    b = np.zeros(90, np.uint8)

    def put(pc, squares):
        free = [s for s in squares if b[s] == 0]
        if free:
            b[free[rs.randint(len(free))]] = pc

    def palace(red):
        return [f + 9 * r for r in (range(0, 3) if red else range(7, 10)) for f in range(3, 6)]

    def base(red):
        return 0 if red else 8
    att, dfn = bool(turn), not bool(turn)
    put(7 + base(att), palace(att))
    put(7 + base(dfn), palace(dfn))
    far = [s for s in range(90) if (s // 9 >= 4) == att]          # the defender's half and the river ranks next to it
    for pc in rs.choice([3, 3, 2, 2, 4, 4, 1, 1], size=rs.randint(2, 5), replace=False):
        put(int(pc) + base(att), far if pc == 1 or rs.rand() < 0.7 else list(range(90)))
    adv = [sq(x) for x in (("d0", "f0", "e1", "d2", "f2") if dfn else ("d9", "f9", "e8", "d7", "f7"))]
    bis = [sq(x) for x in (("c0", "g0", "a2", "e2", "i2", "c4", "g4") if dfn else ("c9", "g9", "a7", "e7", "i7", "c5", "g5"))]
    for pc in rs.choice([6, 6, 5, 5, 3, 4, 2, 1], size=rs.randint(0, 5), replace=False):
        if pc == 6:
            put(6 + base(dfn), adv)
        elif pc == 5:
            put(5 + base(dfn), bis)
        else:
            put(int(pc) + base(dfn), [s for s in range(90) if pc != 1 or (s // 9 <= 6 if not dfn else s // 9 >= 3)])
    return b, turn


def legal_start(b, turn):
    if OracleBoard.from_array(b, turn ^ 1).in_check():         # the side that just moved may not stand in check
        return False
    o = OracleBoard.from_array(b, turn)
    return bool(o.legal_ids()) and not o.is_tie()


def fixture(name, b, turn, halfmove=0, history=(), budgets=(), note=""):
    return {"name": name, "placement": {name_of(s): int(b[s]) for s in range(90) if b[s]}, "turn": int(turn), "halfmove": int(halfmove),
            "history": list(history), "budgets": [int(x) for x in budgets], "note": note}


def main():
    rs = np.random.RandomState(20261021)
    out = [fixture("two_rooks", STARTS["two_rooks"], 1, note="Ra7-a9 mates"),
           fixture("mate_in_two", np.asarray(mc.MATE_IN_TWO), 1, note="i7i8, Kf9 forced, i8i9"),
           fixture("wide_late_mate", STARTS["wide_late_mate"], 1, note="105 legal moves, the only mating move a5a9 at index 67")]
    want = {("dist", d, t): 2 for d in (1, 3, 5, 7) for t in (0, 1)}
    want.update({"state2": 8, "small": 2, "history": 2, "clock": 1, "discovered": 1, "double": 1, "capture": 1})
    tries = 0
    while any(v > 0 for v in want.values()) and tries < 200000 and len(out) < 70:
        tries += 1
        b, turn = random_position(rs)
        if not legal_start(b, turn):
            continue
        o = OracleBoard.from_array(b, turn)
        st, dist, mv, nodes = mm.mate_search(o, PLIES, BIG)
        tags = mc.tags_of(o, st, dist, mv) if st == mm.FOUND else set()
        took = None
        if st == mm.FOUND:
            for t in ("discovered", "double", "capture"):
                if t in tags and want[t] > 0:
                    want[t] -= 1
                    took = t
            if want[("dist", dist, turn)] > 0:
                want[("dist", dist, turn)] -= 1
                took = took or f"dist{dist}"
            small = max(2, nodes // 2)
            if took is None and dist >= 5 and nodes > 40 and want["small"] > 0:
                want["small"] -= 1
                took = "small"
            if took:
                out.append(fixture(f"h{len(out):02d}_{took}", b, turn, budgets=[small] if took == "small" or dist >= 5 else [],
                                   note=f"{took}: mate in {dist} plies, {nodes} nodes"))
            # the same placement at clock 119: the first non-zeroing check reaches 120
            if dist >= 3 and want["clock"] > 0:
                if mm.mate_search(OracleBoard.from_array(b, turn, 119), PLIES, BIG)[0] == mm.NO_MATE:
                    want["clock"] -= 1
                    out.append(fixture(f"h{len(out):02d}_clock", b, turn, halfmove=119, note="clock 119: blocked; the same placement at clock 0 mates"))
            # a history that holds the position after the first move pair of the mating line: reached by taking both moves back
            if dist == 3 and want["history"] > 0:
                h = history_variant(o, mv)
                if h is not None:
                    want["history"] -= 1
                    out.append(fixture(f"h{len(out):02d}_history", h[0], turn, history=h[1], note="the history holds a position of the "
                                       f"3-ply mate: with it {h[2]}, without it mate in 3"))
        elif st == mm.NO_MATE and want["state2"] > 0 and nodes > (PLIES + 1) // 2:     # (more than the four roots: a check exists)
            want["state2"] -= 1
            out.append(fixture(f"h{len(out):02d}_nomate", b, turn, note=f"checks exist, no checking mate within {PLIES} plies, {nodes} nodes"))
    missing = {str(k): v for k, v in want.items() if v > 0}
    print(f"{tries} positions tried, {len(out)} fixtures, missing {missing}", file=sys.stderr)
    json.dump(out, sys.stdout, indent=0)


def history_variant(o, mv):
    """For a 3-ply mate with first move ``mv``: a defender reply d and the position Q after (mv, d) such that Q -mv^-1-> . -d^-1-> P is
    legal and quiet. Returns (Q's squares, [mv^-1, d^-1] in UCI, what the model says with the history) where that differs from mate in 3."""
    L = lib()
    a = o.copy()
    a.push_id(mv)
    for d in a.legal_ids():
        q = a.copy()
        q.push_id(d)
        back_a = L.xq_move_id(L.xq_move_to(mv), L.xq_move_from(mv))
        back_d = L.xq_move_id(L.xq_move_to(d), L.xq_move_from(d))
        if back_a < 0 or back_d < 0:
            continue
        start = OracleBoard.from_array(q.squares(), int(q.turn))
        if back_a not in start.legal_ids() or start.squares()[L.xq_move_from(mv)] != 0:
            continue
        start.push_id(back_a)
        if back_d not in start.legal_ids() or start.squares()[L.xq_move_from(d)] != 0:
            continue
        start.push_id(back_d)
        if not np.array_equal(start.squares(), o.squares()) or start.halfmove != 2 or start.is_tie():
            continue
        got = mm.mate_search(start, PLIES, BIG)
        if got[0] != mm.FOUND or got[1] > 3:
            what = f"mate in {got[1]}" if got[0] == mm.FOUND else "no mate"
            return q.squares(), [L.xq_move_uci(back_a).decode(), L.xq_move_uci(back_d).decode()], what
    return None


if __name__ == "__main__":
    main()
