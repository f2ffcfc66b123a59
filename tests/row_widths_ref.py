"""The row widths (embed_size, and every table row the row kernels see) the width tests run, and what each is for.

The row kernels pick their form from the width W (csrc/segreduce.h: seg_reduce_launch, csrc/optim.hip: mapx_table_adam):
LG = 4, 8 or 16 lanes per row for W <= 16, <= 32 and above, one float4 column per lane; lanes idle when W < 4 LG; a
second column round runs when W > 64.

    4, 8, 12    LG 4, 3 / 2 / 1 idle lanes          36, 40    LG 16, partial        128    two full rounds
    (16: LG 4, full, is what the golden  64        LG 16, full           256    the stated maximum, four rounds
     fixtures and every older test run)
    20, 24      LG 8, partial                       68        two rounds, the second with one live lane
"""
import torch

ROW_WIDTHS = (4, 8, 12, 20, 24, 36, 40, 64, 68, 128, 256)
BF16_ROW_WIDTHS = tuple(W for W in ROW_WIDTHS if W % 8 == 0)     # bf16 compute mode: embed_size % 8 == 0
MAX_ROW_WIDTH = 256

WAVE = 64
SEG_SMALL_N = 1 << 18        # csrc/segreduce.h: kSegSmallN, kSegChunkSmall, kSegChunk
PASS_B_DEPTH = 16            # loads in flight per lane group in pass B's deepest loop (NF)


def lane_group(W):
    return 4 if W <= 16 else (8 if W <= 32 else 16)


def form(W):
    """-> (LG, 'partial' | 'full' | 'rounds') as the commit message and DESIGN.md name the instantiations."""
    lg = lane_group(W)
    return lg, ("rounds" if W > 4 * lg else ("full" if W == 4 * lg else "partial"))


def seg_chunk(n):
    return 16 if n <= SEG_SMALL_N else 32


def deep_loop_chunks(W):
    """Chunks a run must span for pass B's 16-deep loop to run once: G = 64 / LG lane groups share the run."""
    return PASS_B_DEPTH * (WAVE // lane_group(W)) + 1


HOT_KEY = 3


def skewed_keys(n, V, seed):
    """tests/test_kernels_gpu.py::_skewed_keys: a power-law draw plus one hot key on n / 4 positions."""
    g = torch.Generator().manual_seed(seed)
    k = (torch.rand(n, generator=g) ** 6 * V).long().clamp_(0, V - 1)
    k[: n // 4] = HOT_KEY
    return k[torch.randperm(n, generator=g)]


def seg_sizes():
    """(W, n, V) of the reduction cases: every width at n = 33 and 20 000 (V <= n / 50: the hot run spans 312 chunks
    of 16), widths 12 / 40 / 68 also at 2^18 + 1, the first size with the 32-position chunk."""
    out = [(W, n, V) for W in ROW_WIDTHS for n, V in ((33, 7), (20000, 400))]
    return out + [(W, SEG_SMALL_N + 1, 5000) for W in (12, 40, 68)]
