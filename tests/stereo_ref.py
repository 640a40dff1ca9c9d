"""Plain-Python restatement of the epipolar stereo matcher (no GPU, no oracle): CorrespondenceFinderDescriptorBasedEpipolar::compute
(registration/correspondence_finders/correspondence_finder_descriptor_based_epipolar_impl.cpp:46-219) for frames of a few hundred
keypoints.  It keeps the reference's float32 bookkeeping (best / second best start at FLT_MAX, the acceptance test divides in
float32) and the two canonicalisations the C oracle documents: equal (row, col) keys are ordered by unsorted index, and the
scan's bound is tested before its row.  tests/test_stereo_ref.py holds it against the C oracle at the parameter edges the GPU
tables lean on."""
import numpy as np

from stereo_dispatch import FLT_MAX, _features

WARN_EMPTY_INPUT, WARN_NO_MATCHES, WARN_LOW_RATIO = 1, 2, 4


def hamming_matrix(desc_left, desc_right):
    dl = np.ascontiguousarray(desc_left, dtype=np.uint8).reshape(-1, 32)
    dr = np.ascontiguousarray(desc_right, dtype=np.uint8).reshape(-1, 32)
    if len(dl) == 0 or len(dr) == 0:
        return np.zeros((len(dl), len(dr)), dtype=np.int64)
    return np.unpackbits(dl[:, None, :] ^ dr[None, :, :], axis=2).sum(axis=2).astype(np.int64)


def match(uv_left, desc_left, uv_right, desc_right, max_dist, ratio, min_ratio, max_disp, thickness, passes=False):
    """-> (list of (fixed_idx, moving_idx, response), warning flags[, unsorted left indices matched in each pass])"""
    D = hamming_matrix(desc_left, desc_right)
    L, R = _features(uv_left), _features(uv_right)
    n_left = len(L)
    max_dist, ratio = np.float32(max_dist), np.float32(ratio)
    offsets = [0]
    for k in range(1, 1 + max(int(thickness), 0)):
        offsets += [k, -k]
    out, per_pass = [], []
    for off in offsets:
        ir = 0
        matched_l, matched_r = set(), set()
        il = 0
        while il < len(L):
            if ir == len(R):
                break
            # right keypoints on a higher row: advance left
            while L[il][0] + off < R[ir][0]:
                il += 1
                if il == len(L):
                    break
            if il == len(L):
                break
            row_l, col_l, idx_l = L[il][0] + off, L[il][1], L[il][2]
            # right keypoints on a lower row: advance right
            while row_l > R[ir][0]:
                ir += 1
                if ir == len(R):
                    break
            if ir == len(R):
                break
            best, second, ib = FLT_MAX, FLT_MAX, 0
            s = ir
            while s < len(R) and R[s][0] == row_l:
                disparity = col_l - R[s][1]
                if disparity < 0:
                    break
                if disparity > max_disp:
                    s += 1
                    continue
                d = np.float32(D[idx_l, R[s][2]])
                if d < best:
                    second, best, ib = best, d, s
                elif d < second:
                    second = d
                s += 1
            with np.errstate(divide="ignore", invalid="ignore"):
                accept = best < max_dist and np.float32(best / second) < ratio
            if accept:
                out.append((idx_l, R[ib][2], float(best)))
                ir = ib + 1
                matched_l.add(il)
                matched_r.add(ib)
            il += 1
        per_pass.append(sorted(L[k][2] for k in matched_l))
        L = [f for k, f in enumerate(L) if k not in matched_l]
        R = [f for k, f in enumerate(R) if k not in matched_r]
    flags = 0
    if n_left == 0 or len(uv_right) == 0:
        flags |= WARN_EMPTY_INPUT
    if not out:
        flags |= WARN_NO_MATCHES
    with np.errstate(divide="ignore", invalid="ignore"):
        if np.float32(len(out)) / np.float32(n_left) < np.float32(min_ratio):
            flags |= WARN_LOW_RATIO
    return (out, flags, per_pass) if passes else (out, flags)


def as_tuples(corr):
    """a CORR_DTYPE array as the list match() returns"""
    return [(int(c["fixed_idx"]), int(c["moving_idx"]), float(c["response"])) for c in corr]


# ---- inputs that reach chosen paths --------------------------------------------------------------------------------------------
def at_distance(rng, base, d):
    """a copy of descriptor base [32] u8 with exactly d of its 256 bits flipped"""
    bits = np.unpackbits(np.asarray(base, dtype=np.uint8))
    bits[rng.choice(256, int(d), replace=False)] ^= 1
    return np.packbits(bits)


class FrameBuilder:
    """a stereo pair assembled window by window; build() permutes both sides (the unsorted indices are not the sorted order)"""

    def __init__(self, rng):
        self.rng = rng
        self.uvl, self.dl, self.uvr, self.dr = [], [], [], []

    def left(self, u, v, desc):
        self.uvl.append((u, v))
        self.dl.append(desc)
        return len(self.uvl) - 1

    def right(self, u, v, desc):
        self.uvr.append((u, v))
        self.dr.append(desc)
        return len(self.uvr) - 1

    def window(self, row, col, dists, keep=True, v_left=0.5):
        """one left keypoint at column col of row `row` and, right of it, one right keypoint per distance at columns col, col - 1, ..
        (all inside a disparity window of len(dists) - 1 pixels); keep=False puts the right keypoints below the left one (the stereo
        adaptor drops the match).  Returns the left keypoint's builder index."""
        base = self.rng.integers(0, 256, 32, dtype=np.uint8)
        i = self.left(col + 0.5, row + v_left, base)
        for j, d in enumerate(dists):
            self.right(col - j + 0.25, row + (0.25 if keep else 0.75), at_distance(self.rng, base, d))
        return i

    def build(self):
        pl, pr = self.rng.permutation(len(self.uvl)), self.rng.permutation(len(self.uvr))
        uvl = np.asarray(self.uvl, dtype=np.float32).reshape(-1, 2)
        uvr = np.asarray(self.uvr, dtype=np.float32).reshape(-1, 2)
        dl = np.asarray(self.dl, dtype=np.uint8).reshape(-1, 32)
        dr = np.asarray(self.dr, dtype=np.uint8).reshape(-1, 32)
        self.left_index = np.argsort(pl)  # builder index -> unsorted index
        return {"uv_left": uvl[pl], "desc_left": dl[pl], "uv_right": uvr[pr], "desc_right": dr[pr]}


def crowded_frame(rng, rows, n_rows, left_per_row, right_per_row, span, n_bank=6, flip=0.04, jitter=0.0, row_list=None, col0=None):
    """rows full of keypoints: right columns drawn from [c0, c0 + span), left columns from [c0, c0 + span + 8), descriptors drawn
    from a small bank of base rows (several near-equal candidates per window: the ratio test decides); jitter moves that fraction of
    the right keypoints one row up or down (later passes of a thick epipolar line find them); col0 puts every row's keypoints on the
    same columns (a left keypoint then has crowded windows on the rows next to its own too)"""
    used = np.asarray(row_list) if row_list is not None else rng.choice(rows, n_rows, replace=False)
    bank = rng.integers(0, 256, (n_bank, 32), dtype=np.uint8)
    uvl, uvr = [], []
    for r in used:
        c0 = int(rng.integers(0, 1100)) if col0 is None else col0
        ul = rng.integers(c0, c0 + span + 8, left_per_row) + rng.random(left_per_row) * 0.9
        ur = rng.integers(c0, c0 + span, right_per_row) + rng.random(right_per_row) * 0.9
        vr = np.full(right_per_row, r + 0.5)
        if jitter > 0:
            move = rng.random(right_per_row) < jitter
            vr = np.clip(vr + move * rng.choice([-1.0, 1.0], right_per_row), 0.0, rows - 0.5)
        uvl += list(zip(ul, np.full(left_per_row, r + 0.5)))
        uvr += list(zip(ur, vr))
    nl, nr = len(uvl), len(uvr)
    dl = np.bitwise_xor(bank[rng.integers(0, n_bank, nl)], np.packbits(rng.random((nl, 256)) < flip, axis=1))
    dr = np.bitwise_xor(bank[rng.integers(0, n_bank, nr)], np.packbits(rng.random((nr, 256)) < flip, axis=1))
    pl, pr = rng.permutation(nl), rng.permutation(nr)
    return {"uv_left": np.asarray(uvl, np.float32)[pl], "desc_left": dl[pl], "uv_right": np.asarray(uvr, np.float32)[pr], "desc_right": dr[pr]}
