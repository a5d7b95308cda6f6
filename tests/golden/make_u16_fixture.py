"""A hand-assembled IVFADC.jl index file with UInt16 codes (k = 300 > 256), written field by field in the order of the reference's writer
(persistency.jl:22-78): header lines, centroids column by column, per codebook its labels (2 bytes each) then vectors row j across the k
codewords, the identity rotation, per list clsize::Int64, UInt32 ids, then every vector's m UInt16 codes.  Labels are a permutation of
65536 values (not 0..k-1), one list is empty.

    python tests/golden/make_u16_fixture.py      # rewrites tests/golden/persistency_u16_codes.bin
"""
import os
import struct

NROWS, NCLUSTERS, M, K, DSUB = 4, 3, 2, 300, 2
LIST_SIZES = (5, 0, 4)
N = sum(LIST_SIZES)


def centroid(row, col):          # coarse_quantizer.vectors[row, col], 1-based
    return 1.0 * col + 0.25 * row


def codeword(i, j, c):           # residual_quantizer.codebooks[i].vectors[j, c], 1-based
    return ((37 * c + 11 * j + 5 * i) % 101) / 64.0 - 0.75


def label(i, c):                 # codebooks[i].codes[c], 1-based: distinct within a block, spread over 0..65535
    return (c * 217 + 1000 * i) % 65536


def list_id(i, j):
    return 10 * i + j


def list_code(i, j, ii):
    return label(ii, ((7 * i + 13 * j + 3 * ii) % K) + 1)


def main():
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "persistency_u16_codes.bin")
    b = bytearray()
    b += ("%d %d\n%d %d %d %d\nNaiveQuantizer\nQuantizedArrays.OrthogonalQuantization\nUInt16\nUInt32\n"
          "Distances.SqEuclidean\nDistances.SqEuclidean\nFloat32\n" % (NROWS, NCLUSTERS, N, M, K, DSUB)).encode()
    for col in range(1, NCLUSTERS + 1):
        for row in range(1, NROWS + 1):
            b += struct.pack("<f", centroid(row, col))
    for i in range(1, M + 1):
        for c in range(1, K + 1):
            b += struct.pack("<H", label(i, c))
        for j in range(1, DSUB + 1):
            for c in range(1, K + 1):
                b += struct.pack("<f", codeword(i, j, c))
    for col in range(1, NROWS + 1):
        for row in range(1, NROWS + 1):
            b += struct.pack("<f", 1.0 if row == col else 0.0)
    for i in range(1, NCLUSTERS + 1):
        n = LIST_SIZES[i - 1]
        b += struct.pack("<q", n)
        for j in range(1, n + 1):
            b += struct.pack("<I", list_id(i, j))
        for j in range(1, n + 1):
            for ii in range(1, M + 1):
                b += struct.pack("<H", list_code(i, j, ii))
    open(out, "wb").write(bytes(b))


if __name__ == "__main__":
    main()
