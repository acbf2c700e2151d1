"""The bit interleaver's definition (include/polarldpc.h at pl_interleave_check) as plain Python loops: fill
the cells, read the columns.  Independent of the package and of the closed forms.  For sizes no loop can
afford there is ByColumns: the valid cells of the earlier columns, counted from the row starts, plus the
row index."""
import bisect
import math

RECT_ROWS = (1, 2, 3, 4, 6, 8, 10, 64)


def tri_T(E):
    """the smallest T with T (T + 1) / 2 >= E"""
    T = 0
    while T * (T + 1) // 2 < E:
        T += 1
    return T


def row_starts(kind, rows, E):
    """(starts, lengths) of the rows of the array e is written into, empty cells included"""
    if kind == "rect":
        C = -(-E // rows)
        return [r * C for r in range(rows)], [C] * rows
    T = tri_T(E)
    starts, k = [], 0
    for i in range(T):
        starts.append(k)
        k += T - i
    return starts, [T - i for i in range(T)]


def output_order(kind, rows, E):
    """the list of input indices in output order: out[p] = the k with pos(k) = p"""
    starts, lengths = row_starts(kind, rows, E)
    cells = []
    for st, n in zip(starts, lengths):  # write row by row
        cells.append([k if k < E else None for k in range(st, st + n)])
    out = []
    for c in range(max(lengths)):  # read column by column, c outer and r inner
        for row in cells:
            if c < len(row) and row[c] is not None:
                out.append(row[c])
    return out


def positions(kind, rows, E):
    """pos as a list: f[pos[k]] = e[k]"""
    pos = [None] * E
    for p, k in enumerate(output_order(kind, rows, E)):
        pos[k] = p
    return pos


def interleave(kind, rows, e):
    return [e[k] for k in output_order(kind, rows, len(e))]


def deinterleave(kind, rows, f):
    pos = positions(kind, rows, len(f))
    return [f[pos[k]] for k in range(len(f))]


class ByColumns:
    """pos(k) of a large (kind, rows, E) without a table of E entries, from the row starts alone (at most
    46 341 of them): the valid cells before column c, plus the row index.  TRI counts them column by column,
    each column by a binary search over the row starts.  A RECT array of 2^30 cells has 10^8 columns and at
    most 64 rows, so there the same cells are counted row by row: row r holds min(C, E - r C) valid cells,
    clamped at 0, and min(c, that) of them lie before column c."""

    def __init__(self, kind, rows, E):
        self.kind, self.E = kind, E
        if kind == "rect":
            self.C = -(-E // rows)
            self.starts = [r * self.C for r in range(rows)]
        else:
            T = (math.isqrt(8 * E) + 1) // 2
            while T * (T + 1) // 2 < E:
                T += 1
            while T > 1 and (T - 1) * T // 2 >= E:
                T -= 1
            self.T = T
            self.starts, k = [], 0
            for i in range(T):
                self.starts.append(k)
                k += T - i
            self.prefix = [0]  # prefix[c] = valid cells of the columns 0 .. c-1
            for c in range(T):
                n = bisect.bisect_left(self.starts, E - c)  # rows with starts[i] + c < E
                self.prefix.append(self.prefix[-1] + min(n, T - c))  # column c has rows 0 .. T-1-c

    def cell(self, k):
        i = bisect.bisect_right(self.starts, k) - 1
        return i, k - self.starts[i]

    def before(self, c):
        if self.kind == "tri":
            return self.prefix[c]
        return sum(min(c, max(0, min(self.C, self.E - st))) for st in self.starts)

    def pos(self, k):
        i, c = self.cell(k)
        return self.before(c) + i
