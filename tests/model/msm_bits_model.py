"""Host model of the MSM over bounded scalars (csrc/msm_plan.hpp: msm_bound_slices): the rule that picks the slices, the offset tables
the library makes, and the scalars that stress a bound.  Next to msm_sort_model.py, which it leaves alone."""
from msm_sort_model import balanced_slice_offsets

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
BITS_WHOLE = 255      # from here on a bound says nothing (r < 2^255): the entries are the unbounded ones
BITS_GLV_ONE_SET = 127  # split planes: up to here one plain bucket set (lambda > 2^127)


def bound_slices(off, bits):
    """Slices of the offset table `off` (nslice + 1 offsets) that canonical values below 2^bits fill: the smallest t with
    off[t] >= bits + 1, at most nslice."""
    nslice = len(off) - 1
    t = 1
    while t < nslice and off[t] < bits + 1:
        t += 1
    return t


def library_tables():
    """(name, offsets) of every table: per-window 8 and 16, expansions of whole scalars and of the split halves for 9..24-bit windows."""
    tabs = [(f"per-window {c}", [s * c for s in range(256 // c + 1)]) for c in (8, 16)]
    for cover in (256, 129):
        tabs += [(f"expansion {cover}/{w}", balanced_slice_offsets(cover, w)) for w in range(9, 25)]
    return tabs


def handle_table(kind, n):
    """The full offset table of a handle as the GPU tests make them: None (per-window, the automatic width for n terms), or the
    window_bits of zkp_g1_bases_precompute / ("glv", window_bits) of zkp_g1_bases_precompute_glv."""
    if kind is None:
        c = 16 if n >= 2048 else 8
        return [s * c for s in range(256 // c + 1)]
    if isinstance(kind, tuple):
        return balanced_slice_offsets(129, kind[1])
    return balanced_slice_offsets(256, kind)


def edge_values(off, bits):
    """Values below 2^bits that stress the carry over the slices of `off` (already cut to the slices the bound leaves): 0, 1,
    2^(bits - 1), 2^bits - 1, and every slice exactly half its range -- the largest digit that does not carry -- cut to the bound."""
    half = sum(1 << (off[s + 1] - 1) for s in range(len(off) - 1))
    return [0, 1, 1 << (bits - 1), (1 << bits) - 1, half & ((1 << bits) - 1)]
