"""numpy restatement of the speckle filter (prs_speckle_batch_run; the rule is stated in include/proslam_hip.h, BUILD-DEFINED after
OpenCV's filterSpeckles).  It knows nothing of the kernels' tiles: every valid pixel starts with its own raster index as its label,
takes the least label among the 4-neighbours it is connected to and then the label of the pixel its label names, until nothing
changes; component sizes are a bincount of the labels.  The comparison is one float32 subtraction."""
import numpy as np

F = np.float32
PRS_OK, PRS_ERR_RANGE = 0, -4


def params(max_size=200, max_diff=1.0):
    return dict(max_size=int(max_size), max_diff=F(max_diff))


def links(image, max_diff):
    """(valid [rows, cols], right [rows, cols - 1], down [rows - 1, cols]): right[v, u] says (v, u) and (v, u + 1) are connected"""
    x = np.asarray(image)
    assert x.ndim == 2 and x.dtype in (np.float32, np.uint16)
    with np.errstate(invalid="ignore"):
        valid = x > 0
        xf = x.astype(F)
        # NaN for inf - inf, and a comparison with NaN is false
        right = valid[:, 1:] & valid[:, :-1] & (np.abs(xf[:, 1:] - xf[:, :-1]) <= F(max_diff))
        down = valid[1:, :] & valid[:-1, :] & (np.abs(xf[1:, :] - xf[:-1, :]) <= F(max_diff))
    return valid, right, down


def labels(image, max_diff):
    """int32 [rows, cols]: the least raster index of the pixel's component, -1 for an invalid pixel"""
    valid, right, down = links(image, max_diff)
    rows, cols = valid.shape
    big = rows * cols
    L = np.where(valid, np.arange(big, dtype=np.int64).reshape(rows, cols), big)
    while True:
        before = L.copy()
        N = L.copy()
        N[:, 1:] = np.minimum(N[:, 1:], np.where(right, L[:, :-1], big))
        N[:, :-1] = np.minimum(N[:, :-1], np.where(right, L[:, 1:], big))
        N[1:, :] = np.minimum(N[1:, :], np.where(down, L[:-1, :], big))
        N[:-1, :] = np.minimum(N[:-1, :], np.where(down, L[1:, :], big))
        # a label names a pixel of the same component: take that pixel's label (it is no greater)
        flat = np.append(N.reshape(-1), big)
        L = flat[N.reshape(-1)].reshape(rows, cols)
        if np.array_equal(L, before):
            break
    return np.where(valid, L, -1).astype(np.int32)


def speckle_image(image, companion, p):
    """one image -> dict(image, companion (or None), label, n_kept, n_removed); the inputs are not changed"""
    label = labels(image, p["max_diff"])
    valid = label >= 0
    sizes = np.bincount(label[valid], minlength=label.size)
    removed = valid & (sizes[np.maximum(label, 0)] <= p["max_size"])  # a component has a pixel at least: max_size 0 removes none
    out = np.array(image, copy=True)
    out[removed] = 0
    comp = None
    if companion is not None:
        comp = np.array(companion, copy=True)
        comp[removed] = 0
    return dict(image=out, companion=comp, label=label, n_kept=int((valid & ~removed).sum()), n_removed=int(removed.sum()))


def speckle(images, companions, n_images, p):
    """one sequence: images [frames, rows, cols] float32 or uint16, companions the same shape or None -> dict(status, results: a list
    with a dict per image, None for the images that are not touched)"""
    frames = images.shape[0]
    n = frames if n_images is None else int(n_images)
    if n < 0 or n > frames:
        return dict(status=PRS_ERR_RANGE, results=[None] * frames)
    return dict(status=PRS_OK, results=[speckle_image(images[f], None if companions is None else companions[f], p) if f < n else None
                                        for f in range(frames)])
