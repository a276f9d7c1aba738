"""CPU: the chunk-major G16C activation layout's host helpers (net.py g16c_to_boards / boards_to_g16c / g16_to_g16c / g16c_to_g16)
against the byte formula of include/cczero.h: channel c of position pos of board 16 g + j is element
g * 368640 + (c / 32) * 46080 + (pos * 16 + j) * 32 + c % 32."""
import torch

from chinesechesszero_amd.net import boards_to_g16c, g16_to_g16c, g16c_to_boards, g16c_to_g16


def flat(t):
    return t.permute(0, 2, 3, 1).reshape(-1) if t.dim() == 4 else t.reshape(-1)


def test_boards_to_g16c_and_back():
    for B in (1, 16, 20, 48):
        x = torch.arange(B * 256 * 90, dtype=torch.float32).view(B, 256, 10, 9).contiguous(memory_format=torch.channels_last) + 1.0
        c = boards_to_g16c(x)
        Bp = -(-B // 16) * 16
        assert c.shape == (Bp, 256, 10, 9) and c.is_contiguous(memory_format=torch.channels_last)
        m = flat(c)
        assert m.numel() == Bp * 90 * 256
        g = torch.Generator().manual_seed(B)
        for _ in range(200):
            b, ch, pos = (int(torch.randint(0, n, (1,), generator=g)) for n in (Bp, 256, 90))
            at = (b // 16) * 368640 + (ch // 32) * 46080 + (pos * 16 + b % 16) * 32 + ch % 32
            want = float(x[b, ch, pos // 9, pos % 9]) if b < B else 0.0
            assert float(m[at]) == want, (B, b, ch, pos)
        back = g16c_to_boards(c, B)
        assert back.shape == x.shape and torch.equal(back, x)
        assert torch.equal(g16c_to_boards(c)[B:], torch.zeros(Bp - B, 256, 10, 9))
        x_nchw = x.contiguous()                                         # any memory format of the board-order input
        assert torch.equal(flat(boards_to_g16c(x_nchw)), m)


def test_rows_to_g16c_and_back():
    G = 3
    rows = torch.randn(G * 1440, 256)
    c = g16_to_g16c(rows)
    assert c.shape == rows.shape and torch.equal(g16c_to_g16(c), rows)
    # row p of group g, channel ch
    for g, p, ch in ((0, 0, 0), (1, 77, 100), (2, 1439, 255), (1, 720, 31), (2, 5, 32)):
        assert float(c.reshape(-1)[g * 368640 + (ch // 32) * 46080 + p * 32 + ch % 32]) == float(rows[g * 1440 + p, ch])
    # the 4-D channels-last form the evaluator holds, and the board-order helper on top of it
    x4 = rows.view(G * 16, 10, 9, 256).permute(0, 3, 1, 2)
    c4 = g16_to_g16c(x4)
    assert c4.shape == x4.shape and torch.equal(flat(c4), c.reshape(-1)) and torch.equal(flat(g16c_to_g16(c4)), rows.reshape(-1))
    boards = rows.view(G, 90, 16, 256).permute(0, 2, 1, 3).reshape(G * 16, 10, 9, 256).permute(0, 3, 1, 2)
    assert torch.equal(g16c_to_boards(c4), boards) and torch.equal(flat(boards_to_g16c(boards)), c.reshape(-1))
