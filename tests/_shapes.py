"""Shape lists shared by a fixture and the tests that read it (a plain module:
no fixtures, no test collection)."""

# tests/golden/knn_channels.npz (make_goldens.py knn_channels): the channel
# widths of its clouds — every kNN tier (C <= 4, <= 12, <= 32, <= 64, <= 128)
# at its edges and inside, and every tail (C % 4, C % 8, C % 16) of the
# reference's |x|^2 summation order
KNN_CHANNELS = (1, 2, 4, 5, 7, 8, 12, 13, 16, 17, 24, 31, 32, 33, 40, 100, 127)
