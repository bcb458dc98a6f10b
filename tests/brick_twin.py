"""numpy restatement of the brick skip structure (hsk_dev.h, hsk_create, integrate.hip: mark_brick_negative; extract.hip:
row_brick_mask), written from the rule's text: one bit per brick of (2^bshift)^3 voxels, "has ever held a negative TSDF",
bit = (bz * byn + by) * bxn + bx in 32-bit words, the word count rounded up to a multiple of four; behind them 32 words with
one bit per super-brick of 4^3 bricks, used only while the super-bricks fit them.

A volume is the host array of hsk_download_tsdf: [nzs, Y, X, 2] int16 (tsdf, weight), the stored planes."""
import numpy as np

FLAG_WORDS_MAX = 1024     # the brick edge grows while the brick words exceed this (and X, Y allow it)
SUPER_SHIFT = 2           # log2 of the super-brick edge in bricks
SUPER_WORDS = 32


def _ceil_shift(n, s):
    return (n + (1 << s) - 1) >> s


def flag_words(X, Y, nzs, bshift):
    bits = (X >> bshift) * (Y >> bshift) * _ceil_shift(nzs, bshift)
    return ((bits + 31) // 32 + 3) // 4 * 4


def bshift_of(X, Y, nzs):
    """hsk_create's choice: 3, raised while the field is too long and X and Y stay multiples of the next brick edge"""
    bs = 3
    while flag_words(X, Y, nzs, bs) > FLAG_WORDS_MAX and bs < 6 and X % (1 << (bs + 1)) == 0 and Y % (1 << (bs + 1)) == 0:
        bs += 1
    return bs


def super_dim(voxels, bshift):
    return _ceil_shift(voxels >> bshift, SUPER_SHIFT)


def super_count(X, Y, nzs, bshift):
    return super_dim(X, bshift) * super_dim(Y, bshift) * _ceil_shift(_ceil_shift(nzs, bshift), SUPER_SHIFT)


def super_ok(X, Y, nzs, bshift):
    return super_count(X, Y, nzs, bshift) <= SUPER_WORDS * 32


def flag_words_total(X, Y, nzs, bshift):
    return flag_words(X, Y, nzs, bshift) + SUPER_WORDS


def layout(X, Y, nzs):
    """-> dict(bshift, bxn, byn, bzn, words, supers, super_ok, total_words) of a context that stores nzs planes"""
    bs = bshift_of(X, Y, nzs)
    return dict(bshift=bs, bxn=X >> bs, byn=Y >> bs, bzn=_ceil_shift(nzs, bs), words=flag_words(X, Y, nzs, bs),
                supers=super_count(X, Y, nzs, bs), super_ok=super_ok(X, Y, nzs, bs), total_words=flag_words_total(X, Y, nzs, bs))


def brick_bits(vol, bshift=None):
    """the bricks that must be set: [bzn, byn, bxn] bool, True where a voxel of the brick has F < 0"""
    nzs, Y, X, _ = vol.shape
    bs = bshift_of(X, Y, nzs) if bshift is None else bshift
    e = 1 << bs
    bzn = _ceil_shift(nzs, bs)
    neg = np.zeros((bzn * e, Y, X), bool)
    neg[:nzs] = vol[..., 0] < 0
    return neg.reshape(bzn, e, Y >> bs, e, X >> bs, e).any(axis=(1, 3, 5))


def super_bits(bricks):
    """the super-bricks of a brick array: [szn, syn, sxn] bool"""
    s = 1 << SUPER_SHIFT
    bzn, byn, bxn = bricks.shape
    pad = np.zeros((_ceil_shift(bzn, SUPER_SHIFT) * s, _ceil_shift(byn, SUPER_SHIFT) * s, _ceil_shift(bxn, SUPER_SHIFT) * s), bool)
    pad[:bzn, :byn, :bxn] = bricks
    return pad.reshape(pad.shape[0] // s, s, pad.shape[1] // s, s, pad.shape[2] // s, s).any(axis=(1, 3, 5))


def _pack(bits, words):
    out = np.zeros(words, np.uint32)
    idx = np.flatnonzero(bits.reshape(-1))
    np.bitwise_or.at(out, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
    return out


def field(vol):
    """the whole field a rebuild of `vol` leaves: the brick words, then the SUPER_WORDS super-brick words (all zero when the
    super-bricks do not fit them) -> uint32 [total_words]"""
    nzs, Y, X, _ = vol.shape
    L = layout(X, Y, nzs)
    b = brick_bits(vol, L["bshift"])
    sup = _pack(super_bits(b), SUPER_WORDS) if L["super_ok"] else np.zeros(SUPER_WORDS, np.uint32)
    return np.concatenate([_pack(b, L["words"]), sup])


def row_span(bz, by, bxn, byn):
    """where brick row (bz, by) starts in the field -> (w0, sh): its first bit is bit sh of word w0"""
    bit0 = (bz * byn + by) * bxn
    return bit0 >> 5, bit0 & 31


def third_word_bricks(bricks):
    """the set bricks whose bit a reader of a row's (at most) three words takes from the third: rows with sh != 0 and
    sh + bxn > 64, brick index >= 64 - sh -> list of (bz, by, bx)"""
    bzn, byn, bxn = bricks.shape
    out = []
    for bz in range(bzn):
        for by in range(byn):
            _, sh = row_span(bz, by, bxn, byn)
            if sh != 0 and sh + bxn > 64:
                out += [(bz, by, int(bx)) for bx in np.flatnonzero(bricks[bz, by]) if bx >= 64 - sh]
    return out


def set_bits_beyond_word(bricks, word):
    """the number of set brick bits that live in words >= `word`"""
    idx = np.flatnonzero(bricks.reshape(-1))
    return int(((idx >> 5) >= word).sum())
