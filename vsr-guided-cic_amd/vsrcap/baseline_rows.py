"""The row layout of a sampling call with a greedy baseline row per image (include/vsrcap.h, vsr_sample_rows_baseline), stated once on
the host.  No torch, no ctypes: the engine sizes and checks its tensors with it and the CPU tests hold it to the header's rule.

K samples per image: the decoder runs K + 1 adjacent rows per image, the baseline first.  The baseline of image b lands in row b of the
(B, T) baseline outputs; sample j of image b in row b K + j of the (B K, T) sample tensors - the row it has in the samples_per_image=K
call without a baseline, the order of repeat_interleave(K, 0).  That index is also its noise key and the row of its forced ids.
"""


def decoder_row(row, samples_per_image):
    """decoder row of the (K + 1)-rows-per-image layout -> ("baseline", b) or ("sample", b * K + j)"""
    K = int(samples_per_image)
    if K < 1 or row < 0:
        raise ValueError("decoder_row: row %r of a call with %r samples per image" % (row, samples_per_image))
    gs = K + 1
    b, r = divmod(int(row), gs)
    if r == 0:
        return ("baseline", b)
    return ("sample", row - row // gs - 1)          # = b * K + (r - 1); the kernels' form (csrc/kernels.h, sample_row)


def output_rows(images, samples_per_image):
    """(rows of the sample tensors, rows of the baseline tensors) of a call on `images` images: one past the destination of the last
    decoder row of either kind"""
    if images <= 0:
        return 0, 0
    gs = int(samples_per_image) + 1
    kind_s, last_sample = decoder_row(images * gs - 1, samples_per_image)
    kind_b, last_base = decoder_row((images - 1) * gs, samples_per_image)
    assert kind_s == "sample" and kind_b == "baseline"
    return last_sample + 1, last_base + 1
