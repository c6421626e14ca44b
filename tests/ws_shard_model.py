"""Numpy models of what a rank of a sharded working-set round must leave, written from the rules (ws_common.hpp
"peer exchange", ws_merge.hip ws_gather_row, device_state.hpp WsArgs), not from the kernels: the shard of a rank,
the selection geometry, the owner mask of a gather, a rank's candidate lists with global row indices, the
line-search partials' slots, and the exchange region's slot offsets and tag.  Their own invariants:
test_ws_shard_model_cpu.py; the kernels against them: test_ws_shard_kernels_gpu.py."""
import numpy as np

from test_ws_kernels_gpu import KC, KC1, NONE, make_key

M48 = (1 << 48) - 1


def shard_of(n, r, W):
    """(off, nl) of rank r: the first n % W ranks hold one row more (common.hpp shard_of)"""
    base, rem = divmod(n, W)
    return r * base + min(r, rem), base + (1 if r < rem else 0)


def geometry(n, W):
    """(G, rpt) every rank uses: <= min(256, 1024 // W) workgroups of 256 threads x rpt rows over the largest shard"""
    nl_max = -(-n // W)
    gmax = max(1, min(256, 1024 // W))
    G = max(1, min(gmax, -(-nl_max // 256)))
    return G, max(1, -(-nl_max // (G * 256)))


def pass1_groups(n, W):
    return max(1, -(-(-(-n // W)) // 1024))


# ---------------------------------------------------------------- gathers
def owner_mask(idx, q, q_max, off, nl):
    """(sub [q_max][q_max], f [q_max]): the entries rank [off, off + nl) fills — (ra, col) with ra, col < q and
    column row idx[col] owned; the f of a row < q it owns.  Everything else it must leave zero."""
    idx = np.asarray(idx, np.int64)
    own = np.zeros(q_max, bool)
    own[:q] = (idx[:q] >= off) & (idx[:q] < off + nl)
    live = np.arange(q_max) < q
    return live[:, None] & own[None, :], own


def gather_model(gram, f, alpha, y, idx, q, q_max, off, nl, lines=None):
    """rank's (subg [q_max][q_max], aux [3][q_max]) from the global gram [L][n] (row ra's kernel row at line
    lines[ra], dense: idx[ra]) and global f / alpha / y"""
    idx = np.asarray(idx, np.int64)
    ln = idx if lines is None else np.asarray(lines, np.int64)
    sub_m, f_m = owner_mask(idx, q, q_max, off, nl)
    sub = np.zeros((q_max, q_max), np.float32)
    aux = np.zeros((3, q_max), np.float32)
    full = gram[ln[:q]][:, idx[:q]]
    sub[:q, :q] = np.where(sub_m[:q, :q], full, np.float32(0))
    aux[0, :q] = np.where(f_m[:q], f[idx[:q]], np.float32(0))
    aux[1, :q] = alpha[idx[:q]]
    aux[2, :q] = y[idx[:q]]
    return sub, aux


# ---------------------------------------------------------------- candidates
def in_sets(a, y, C):
    """(I_up, I_low) membership; C a scalar (the equality form) or an array of per-row bounds (the compare form:
    a row with C_i = 0 is in neither)"""
    a, y = np.asarray(a, np.float32), np.asarray(y, np.float32)
    if np.ndim(C) == 0:
        C = np.float32(C)
        up = np.where(a == 0, y == 1, np.where(a == C, y != 1, True))
        lo = np.where(a == 0, y != 1, np.where(a == C, y == 1, True))
        return up, lo
    C = np.asarray(C, np.float32)
    return np.where(y > 0, a < C, a > 0), np.where(y > 0, a > 0, a < C)


def rank_candidates(f_shard, alpha, y, C, off, G, rpt, nc=KC):
    """[G][2][KC] lists of the rank owning rows [off, off + len(f_shard)): workgroup b holds local rows
    [b rpt 256, (b + 1) rpt 256), its nc smallest keys a side, the key's row index global; the tail kKeyNone"""
    nl = len(f_shard)
    out = np.full((G, 2, KC), NONE, dtype=np.uint64)
    for b in range(G):
        j = np.arange(b * rpt * 256, min(nl, (b + 1) * rpt * 256))
        if len(j) == 0:
            continue
        gj = off + j
        up, lo = in_sets(alpha[gj], y[gj], C if np.ndim(C) == 0 else np.asarray(C)[gj])
        u = np.sort(make_key(f_shard[j][up], gj[up]))[:nc]
        l_ = np.sort(make_key(-f_shard[j][lo], gj[lo]))[:nc]
        out[b, 0, : len(u)] = u
        out[b, 1, : len(l_)] = l_
    return out


def all_candidates(f, alpha, y, C, W, nc=KC):
    """the all-gathered lists [W G][2][KC]: every rank's, in rank order"""
    n = len(f)
    G, rpt = geometry(n, W)
    return np.concatenate([rank_candidates(f[o:o + m], alpha, y, C, o, G, rpt, nc)
                           for o, m in (shard_of(n, r, W) for r in range(W))])


# ---------------------------------------------------------------- partials
def part_slots(r, p1G, ks):
    """the doubles of part [W p1G][ks][2] rank r writes: slot (r p1G + group) ks + slice"""
    return np.arange(2 * r * p1G * ks, 2 * (r + 1) * p1G * ks)


# ---------------------------------------------------------------- exchange region
def xtag(T):
    """granule tag of publication T = round + 1: 16 bits, never 0"""
    return (T % (1 << 32) % 65535 + 1) << 48


def xlayout(blocks, G_all, W, p1G, ks, q_max):
    """(xcw, xpart, xsub, xsub_rows, words) of a rank's receive buffer: [2][G_all][xcw] candidate granules, then
    (multi-block) [2][W p1G ks][4] partials, then [2][xsub_rows][q_max + 1] sub-Gram rows"""
    if blocks > 1:
        xcw = 4 * KC
        xpart = 2 * G_all * xcw
        xsub = xpart + 2 * W * p1G * ks * 4
        rows = blocks * q_max
    else:
        xcw, xpart, rows = 4 * KC1, 0, q_max
        xsub = 2 * G_all * xcw
    return xcw, xpart, xsub, rows, xsub + 2 * rows * (q_max + 1)


def xcand_at(par, slot, side, r, G_all, xcw):
    """first of the two granules of key r, side (0 up, 1 low), of list `slot`"""
    return (par * G_all + slot) * xcw + side * (xcw // 2) + 2 * r


def xpart_at(par, k, xpart, nparts):
    return xpart + (par * nparts + k) * 4


def xrow_at(par, row, col, xsub, xsub_rows, q_max):
    """entry (row, col) of the sub-Gram rows; col = q_max: the row's f"""
    return xsub + (par * xsub_rows + row) * (q_max + 1) + col


def put64(tag, v):
    """a 64-bit payload as two tagged granules (bits 63..16, bits 15..0) ..."""
    return tag | (int(v) >> 16), tag | (int(v) & 0xFFFF)


def get64(g0, g1):
    """... and back"""
    return ((int(g0) & M48) << 16) | (int(g1) & 0xFFFF)
