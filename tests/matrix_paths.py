"""CPU model of which MatrixConvolver kernel paths a shape runs
(fft-convolution_amd/csrc/matrix.hip): geo() mirrors MGeo, matrix_nt and
matrix_b_kernel's UB, parts() the matrix_mac_parts rule, walk() replays
matrix_row_walk (matrix.hpp) over the dense rows for every (part, group).  The
constants are duplicated on purpose: tests/test_matrix_ref.py asserts, for every shape of SHAPES, the
property the shape is there for, so a change of U / G / UB / the P rule fails
with "shape X no longer reaches path Y"; tests/test_gpu_matrix.py asserts that
the library's mac_parts equals the model's P."""
from collections import namedtuple

from matrix_ref import RAGGED_64

Geo = namedtuple("Geo", "NT F G SPT U UB")
Walk = namedtuple("Walk", "R P rpp unrolled tail groups_both max_cross cross_in_unrolled exact "
                          "short_last_part part_chunks input_chunks")


def geo(B):
    """NT, F, G, SPT, U, UB of block size B (a power of two, 32..8192)"""
    log2b = B.bit_length() - 1
    assert 1 << log2b == B and 5 <= log2b <= 13, B
    NT = 256 if log2b <= 10 else 512                    # matrix_nt
    F = B // 2                                          # 16-byte slots per row
    G = 1 if F >= NT else NT // F                       # row groups of a MAC workgroup
    SPT = F // NT if F >= NT else 1                     # slots per thread
    U = {1: 8, 2: 4, 4: 2}.get(SPT, 1)                  # rows in flight (matrix_row_walk)
    UB = {1: 16, 2: 8}.get(SPT, 4)                      # terms in flight (matrix_b_kernel)
    return Geo(NT, F, G, SPT, U, UB)


def parts(I, act):
    """matrix_mac_parts: about 64 rows per part, at most 64 parts"""
    R = I * (act - 1 if act > 1 else 0)
    return min(max((R + 63) // 64, 1), 64)


def walk(B, I, act):
    """matrix_row_walk over every (part, group) of one block with `act` active
    segments: unrolled = iterations of the U-rows-in-flight loop, tail = rows of
    the tail loop, groups_both = groups that run both loops, max_cross = the most
    inputs one advance() steps over, cross_in_unrolled = an unrolled iteration
    whose rows belong to more than one input, exact = every row (i, s), i < I,
    1 <= s < act, is visited exactly once and nothing else is;
    part_chunks / input_chunks = iterations of matrix_b_kernel's two sums."""
    g_ = geo(B)
    G, U, UB = g_.G, g_.U, g_.UB
    am1 = max(act - 1, 0)
    R = I * am1
    P = parts(I, act)
    rpp = -(-R // P)
    seen = {}
    in_range = True
    unrolled = tail = groups_both = max_cross = 0
    cross_in_unrolled = False
    for p in range(P):
        r0 = p * rpp
        r1 = min(r0 + rpp, R)
        for g in range(G):
            r = r0 + g
            i, s = (r // am1, 1 + r % am1) if am1 > 0 else (0, 1)
            it = tl = 0

            def advance():
                nonlocal r, i, s, max_cross
                r += G
                s += G
                crossed = 0
                while s > am1:
                    s -= am1
                    i += 1
                    crossed += 1
                max_cross = max(max_cross, crossed)

            def visit():
                nonlocal in_range
                if not (0 <= i < I and 1 <= s < act and r == i * am1 + s - 1):
                    in_range = False
                seen[(i, s)] = seen.get((i, s), 0) + 1

            while r + (U - 1) * G < r1:
                first = i
                for _ in range(U):
                    visit()
                    if i != first:
                        cross_in_unrolled = True
                    advance()
                it += 1
            while r < r1:
                visit()
                advance()
                tl += 1
            unrolled += it
            tail += tl
            groups_both += 1 if it and tl else 0
    exact = in_range and len(seen) == R and all(v == 1 for v in seen.values())
    return Walk(R, P, rpp, unrolled, tail, groups_both, max_cross, cross_in_unrolled, exact,
                P * rpp > R, -(-P // UB), -(-I // (UB // 2)))


# The shapes of tests/test_gpu_matrix.py::test_paths, minimal under the
# property each is there for; L = S * B - 3 (a ragged last segment), S + 3 full
# blocks so the delay line wraps and every row contributes.  `why` names
# predicates of PROPERTIES, checked on the CPU by tests/test_matrix_ref.py.
Shape = namedtuple("Shape", "B I O S why")
SHAPES = [
    Shape(32, 60, 2, 138, ("capped", "unrolled", "tail", "both", "short_last", "parts>UB", "four_part_chunks",
                           "ragged_inputs", "cross_unrolled")),
    Shape(64, 30, 2, 138, ("capped", "unrolled", "tail", "both", "short_last", "parts>UB", "four_part_chunks",
                           "ragged_inputs", "cross_unrolled")),
    Shape(128, 11, 2, 7, ("unrolled", "tail", "both", "two_parts", "ragged_inputs", "cross_unrolled")),
    Shape(256, 11, 2, 7, ("unrolled", "tail", "both", "two_parts", "ragged_inputs", "cross_unrolled")),
    Shape(512, 11, 2, 7, ("unrolled", "tail", "both", "two_parts", "ragged_inputs", "cross_unrolled")),
    Shape(1024, 5, 2, 14, ("spt2", "nt256", "unrolled", "tail", "both", "two_parts", "ragged_inputs", "cross_unrolled")),
    Shape(2048, 5, 2, 14, ("spt2", "nt512", "unrolled", "tail", "both", "two_parts", "ragged_inputs",
                          "cross_unrolled")),
    Shape(4096, 3, 1, 23, ("spt4", "unrolled", "tail", "both", "two_parts", "ragged_inputs", "cross_unrolled")),
    Shape(8192, 3, 1, 23, ("spt8", "unrolled", "two_parts", "ragged_inputs")),
    Shape(256, 9, 1, 130, ("parts>UB", "unrolled", "tail", "both", "short_last")),
    Shape(1024, 9, 1, 66, ("parts>UB", "unrolled", "tail", "both", "short_last")),
    Shape(4096, 5, 1, 53, ("parts>UB", "unrolled")),
    Shape(32, 41, 2, 2, ("cross_G", "one_part")),
    Shape(64, 20, 2, 2, ("cross_G", "one_part")),
    Shape(64, 20, 2, 3, ("cross_half_G", "one_part")),
    Shape(64, 1, 1, 1, ("no_rows",)),
    Shape(64, 1, 1, 2, ("single_row",)),
]

PROPERTIES = {
    "capped": lambda s, g, w: w.R > 4096 and w.P == 64 and w.rpp > 64,
    "unrolled": lambda s, g, w: w.unrolled > 0,
    "tail": lambda s, g, w: w.tail > 0,
    "both": lambda s, g, w: w.groups_both > 0,
    "short_last": lambda s, g, w: w.short_last_part,
    "two_parts": lambda s, g, w: w.P == 2,
    "one_part": lambda s, g, w: w.P == 1 and w.R > 0,
    "parts>UB": lambda s, g, w: w.P > g.UB and w.part_chunks >= 2,
    "four_part_chunks": lambda s, g, w: w.part_chunks == 4,
    "ragged_inputs": lambda s, g, w: s.I > g.UB // 2 and s.I % (g.UB // 2) != 0,
    "cross_unrolled": lambda s, g, w: w.cross_in_unrolled,
    "spt2": lambda s, g, w: (g.G, g.SPT, g.U, g.UB) == (1, 2, 4, 8),
    "spt4": lambda s, g, w: (g.G, g.SPT, g.U, g.UB) == (1, 4, 2, 4),
    "spt8": lambda s, g, w: (g.G, g.SPT, g.U, g.UB) == (1, 8, 1, 4),
    "nt256": lambda s, g, w: g.NT == 256,
    "nt512": lambda s, g, w: g.NT == 512,
    "cross_G": lambda s, g, w: g.G > 1 and s.S - 1 == 1 and w.max_cross >= g.G,
    "cross_half_G": lambda s, g, w: g.G > 1 and s.S - 1 == 2 and w.max_cross >= g.G // 2,
    "no_rows": lambda s, g, w: w.R == 0 and w.P == 1 and w.unrolled == 0 and w.tail == 0,
    "single_row": lambda s, g, w: w.R == 1 and w.P == 1 and w.tail == 1,
}


def shape_id(s):
    return f"B{s.B}-I{s.I}-O{s.O}-S{s.S}"


def shape_len(s):
    """response length: the last segment is ragged"""
    return s.S * s.B - 3


def shape_blocks(s):
    """full blocks per run: the delay line wraps, every row contributes"""
    return s.S + 3


# ragged call sequences of the two capped shapes (P = 64): one call of S blocks
# that fills the delay line, then calls that start and end anywhere
RAGGED_32 = [1, 7, 32, 50, 3, 100, 32, 33, 64, 15, 17] * 3
CAPPED = [s for s in SHAPES if "capped" in s.why]


def capped_lengths(s):
    return (s.S * s.B,) + tuple({32: RAGGED_32, 64: RAGGED_64}[s.B])
