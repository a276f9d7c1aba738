"""chinesechesszero_amd -- MI355X-native self-play rollout engine for ChineseChessZero.

Only what the hot path needs: the gfx950 HIP engine behind a C ABI
(``csrc/``, ``include/cczero.h``) and the host-side mirror of the reference's call surface
(``tools``, ``parameters``, ``net``, ``mcts``, ``game``, ``collect``) plus the tuple all-gather
(``replay``). There is no CPU fallback: the engine fails loudly when ``libcczero.so`` or a GPU is
missing.
"""
# The package leaves GPU_MAX_HW_QUEUES (the hardware queues HIP maps a process's streams onto) to the environment. The evaluator
# runs its tower as three concurrent launch chains on streams of its own and binds them when the first inference copy is built
# (net.chain_streams), before a process group or the multi-GPU exchange creates streams of theirs; with few queues the chains
# share queues and overlap less.

__version__ = "0.1.0"
