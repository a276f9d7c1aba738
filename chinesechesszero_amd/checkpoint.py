"""Checkpoints of a collecting job (``collect.CollectPipeline``: ``--checkpoint-dir`` / ``--checkpoint-every`` / ``--resume``): the
directory handling, the one definition of the three flags, and the comparison of the options a checkpoint was written with.
Nothing here touches the GPU; what a checkpoint holds is decided by the pipeline.

A checkpoint is ONE file, ``ckpt_<moves, 9 digits>.pt`` (``torch.save``), written under ``<name>.tmp`` and renamed -- as ``TupleSink``
does with its shards -- so a file with the final name is complete; a ``.tmp`` a dead process left is never read. The newest ``KEEP``
are kept. Single rank only: the exchange of a multi-rank job (``replay.AsyncRecordExchange``) has games in flight between the ranks
at every move boundary, and nothing here saves them."""
from __future__ import annotations

import os
import re

KEEP = 2
_NAME = re.compile(r"^ckpt_(\d{9})\.pt$")
MULTI_RANK = ("checkpoints (--checkpoint-dir / --resume) are single-rank: with more than one rank the exchange holds finished games "
              "in flight between the ranks at every move boundary, and a checkpoint does not save them")


def add_checkpoint_args(parser):
    """--checkpoint-dir / --checkpoint-every / --resume."""
    parser.add_argument("--checkpoint-dir", type=str, default=None, help="batched path, one rank: write resumable checkpoints of the whole job "
                        "(games in progress with their trees, replay ring, trainer, sampling generator, the sink's counts) to this directory")
    parser.add_argument("--checkpoint-every", type=int, default=0, help="... one every this many lockstep moves, at the move boundary, after the "
                        "move's harvest reached the sink and the ring (the newest two are kept; needs --checkpoint-dir)")
    parser.add_argument("--resume", action="store_true", default=False, help="continue from the newest complete checkpoint in --checkpoint-dir: "
                        "bit for bit the run that was interrupted; refuses a missing or empty directory and a checkpoint written with other options")


def checkpoint_from_args(parser, a, world: int = 1) -> dict:
    """The checkpoint keywords of ``CollectPipeline(...)``; ``parser.error`` on a flag without its main flag and on several ranks."""
    if (a.checkpoint_every or a.resume) and not a.checkpoint_dir:
        parser.error("--checkpoint-every / --resume need --checkpoint-dir")
    if a.checkpoint_every < 0:
        parser.error(f"--checkpoint-every must not be negative (got {a.checkpoint_every})")
    if a.checkpoint_dir and int(world) > 1:
        parser.error(MULTI_RANK)
    if a.checkpoint_dir and a.boards <= 1:
        parser.error("--checkpoint-dir needs the batched path (--boards > 1)")
    return dict(checkpoint_dir=a.checkpoint_dir, checkpoint_every=a.checkpoint_every, resume=a.resume)


def path_of(directory: str, moves: int) -> str:
    return os.path.join(directory, f"ckpt_{int(moves):09d}.pt")


def complete(directory: str) -> list:
    """``[(moves, path)]`` of the complete checkpoints in ``directory``, oldest first (half-written ``.tmp`` files are not among them)."""
    out = []
    for name in os.listdir(directory):
        m = _NAME.match(name)
        if m:
            out.append((int(m.group(1)), os.path.join(directory, name)))
    return sorted(out)


def write(directory: str, moves: int, payload: dict, keep: int = KEEP) -> str:
    """``payload`` as the checkpoint after ``moves`` lockstep moves: written under a temporary name, renamed, then all but the newest
    ``keep`` complete checkpoints are removed. Returns the path."""
    import torch
    os.makedirs(directory, exist_ok=True)
    path = path_of(directory, moves)
    tmp = path + ".tmp"
    torch.save(payload, tmp)
    os.replace(tmp, path)
    for _, old in complete(directory)[:-keep]:
        os.remove(old)
    return path


def newest(directory: str) -> tuple:
    """``(moves, path)`` of the newest complete checkpoint. A missing directory and one without a complete checkpoint are refused: a
    job asked to resume never silently starts fresh."""
    if not directory or not os.path.isdir(directory):
        raise FileNotFoundError(f"--resume: the checkpoint directory {directory!r} does not exist (start without --resume to begin a new run)")
    found = complete(directory)
    if not found:
        raise FileNotFoundError(f"--resume: {directory} holds no complete checkpoint (start without --resume to begin a new run)")
    return found[-1]


def load_newest(directory: str) -> tuple:
    """``(moves, payload)`` of the newest complete checkpoint (``newest``)."""
    import torch
    moves, path = newest(directory)
    return moves, torch.load(path, map_location="cpu", weights_only=False)


def differences(saved: dict, mine: dict) -> list:
    """What differs between the options a checkpoint was written with and this job's, as ``name: saved != mine`` strings."""
    return [f"{k}: the checkpoint has {saved.get(k)!r}, this job {mine.get(k)!r}" for k in sorted(set(saved) | set(mine)) if saved.get(k) != mine.get(k)]


class RowSkipper:
    """No row twice. A resumed job replays, bit for bit, the moves its dead predecessor played after its last checkpoint, and the sink
    of the data directory already holds what those moves appended. The checkpoint says how many rows the sink held when it was
    written; the resumed sink counts what it finds; the difference is what the replay would append a second time, and exactly that
    many leading rows of the resumed job's appends are dropped. Nothing the sink finds is ever deleted. (Games are not skipped but
    counted again from the checkpoint's count: the counter is a number, not data.)"""

    def __init__(self, rows_at_checkpoint: int, rows_found: int):
        if rows_found < rows_at_checkpoint:
            raise ValueError(f"the data directory holds {rows_found} rows, fewer than the {rows_at_checkpoint} it held when the checkpoint was "
                             "written: rows were removed since, refusing to resume on top of it")
        self.rows = int(rows_found) - int(rows_at_checkpoint)

    def take(self, rows: int) -> int:
        """Of an append of ``rows`` rows: how many leading rows to drop."""
        r = min(int(rows), self.rows)
        self.rows -= r
        return r
