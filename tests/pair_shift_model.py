"""numpy model of the second half of the bottom-aligned HW column (edlib_amd/csrc/reads_column_asm.hpp): from the horizontal
deltas Ph, Mh of a column of NWD 32-row words to the new vertical deltas Pn, Mn and the score delta of the followed row
(bit 31 of the last word), with `<< 1` of the NWD-word vectors written in the two forms the kernel has:

  shift_chain   word 0 as x + x (HW: a zero comes in from row -1), word i as v_alignbit_b32(w[i], w[i-1], 31)
  shift_pairs   the pair schedule: words (0,1), (2,3), (4,5), (6,7) as 64-bit values in register pairs, shifted IN PLACE by
                v_lshlrev_b64 (first pair) or v_lshl_add_u64 pair, pair, 1, {carry, 0} (later pairs; the carry is bit 31 of the
                pair below, taken by v_lshrrev_b32 BEFORE that pair is shifted); a lone last word (odd NWD) by v_alignbit_b32
                from the UNSHIFTED high word of the last pair, so it is issued before that pair's shift.

Arrays are uint32 of shape (n, NWD): n states at once.  The model follows the register schedule (one array updated in place, in
the kernel's order), so that an order mistake -- the lone word fed from an already shifted neighbour -- shows as a wrong word
(`lone_after_pair_shift=True` makes that mistake on purpose)."""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def _u32(x):
    return (np.asarray(x, dtype=np.uint64) & _M32).astype(np.uint32)


def alignbit(hi, lo, sh):
    """v_alignbit_b32: bits [sh, sh + 32) of the 64-bit value hi:lo"""
    v = (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)
    return _u32(v >> np.uint64(sh))


def shift_chain(w):
    w = np.asarray(w, dtype=np.uint32)
    out = np.empty_like(w)
    out[:, 0] = _u32(w[:, 0].astype(np.uint64) + w[:, 0].astype(np.uint64))           # v_add_u32 x, x
    for i in range(1, w.shape[1]):
        out[:, i] = alignbit(w[:, i], w[:, i - 1], 31)
    return out


def shift_pairs(w, lone_after_pair_shift=False):
    r = np.array(w, dtype=np.uint32, copy=True)                  # the registers: shifted in place
    nwd = r.shape[1]
    npairs = nwd // 2
    carry = None                                                 # low half of the (carry, 0) pair
    for k in range(npairs):
        lo, hi = 2 * k, 2 * k + 1
        last_pair = k == npairs - 1
        if last_pair and nwd % 2 and not lone_after_pair_shift:
            r[:, nwd - 1] = alignbit(r[:, nwd - 1], r[:, hi], 31)                      # before the pair is shifted in place
        nxt = r[:, hi] >> np.uint32(31)                          # v_lshrrev_b32: the carry into the next pair
        v = (r[:, hi].astype(np.uint64) << np.uint64(32)) | r[:, lo].astype(np.uint64)
        v = v << np.uint64(1)                                    # 64-bit shift: bit 63 falls off
        if carry is not None:
            v = v + carry.astype(np.uint64)                      # + {carry, 0}: bit 0 is clear after the shift, no carry out
        r[:, lo] = _u32(v)
        r[:, hi] = _u32(v >> np.uint64(32))
        if last_pair and nwd % 2 and lone_after_pair_shift:
            r[:, nwd - 1] = alignbit(r[:, nwd - 1], r[:, hi], 31)                      # the mistake: r[hi] is already shifted
        carry = nxt
    if npairs == 0:                                              # one word: x + x, as the chain
        r[:, 0] = _u32(r[:, 0].astype(np.uint64) << np.uint64(1))
    return r


def column_tail(eq, mv, ph, mh, shift):
    """(Pn, Mn, score delta) of calculateBlock's second half on NWD words, rows bottom-aligned"""
    ph = np.asarray(ph, dtype=np.uint32)
    mh = np.asarray(mh, dtype=np.uint32)
    delta = (ph[:, -1] >> np.uint32(31)).astype(np.int64) - (mh[:, -1] >> np.uint32(31)).astype(np.int64)
    phs, mhs = shift(ph), shift(mh)
    xv = np.asarray(eq, dtype=np.uint32) | np.asarray(mv, dtype=np.uint32)
    pn = mhs | ~(xv | phs)
    mn = phs & xv
    return pn, mn, delta


def edge_patterns(nwd, fill):
    """all 4 ** nwd settings of bit 31 and bit 0 of every word; the 30 bits between are `fill` (0 or 1)"""
    n = 4 ** nwd
    idx = np.arange(n, dtype=np.uint64)
    mid = np.uint32(0x7FFFFFFE if fill else 0)
    out = np.empty((n, nwd), dtype=np.uint32)
    for i in range(nwd):
        b0 = ((idx >> np.uint64(2 * i)) & np.uint64(1)).astype(np.uint32)
        b31 = ((idx >> np.uint64(2 * i + 1)) & np.uint64(1)).astype(np.uint32)
        out[:, i] = mid | b0 | (b31 << np.uint32(31))
    return out
