"""Stand-in for the `editdistance` package the reference's CTC criterion imports (not installed here): eval(a, b) = the Levenshtein
distance of two sequences, by the textbook two-row dynamic programme."""


def eval(a, b):  # noqa: A001  (the package's own name)
    a, b = list(a), list(b)
    row = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        prev, row[0] = row[0], i
        for j in range(1, len(b) + 1):
            cur = min(row[j] + 1, row[j - 1] + 1, prev + (a[i - 1] != b[j - 1]))
            prev, row[j] = row[j], cur
    return row[len(b)]
