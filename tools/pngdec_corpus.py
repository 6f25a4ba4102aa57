"""Writes the PNG reader's test corpus (tests/pngdec_cases.py: the matrix, the IDAT splits, the hand-assembled streams, the refusals,
the corrupt files) into a directory for tools/pngdec_check.cpp: <name>.png and <name>.expect ("<status> <H> <W>\\n", then the gray
bytes PIL gives for a file that decodes).  H x W of a file that does not decode is the output buffer the check hands in."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pngdec_cases as C  # noqa: E402


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    items = [("ok-" + n, d, C.OK, w) for cases in (C.matrix(), C.splits(), C.hand_streams()) for n, d, w in cases]
    items += [("refused-" + n, d, C.EUNSUPPORTED, None) for n, d in C.refusals()]
    items += [("corrupt-" + n, d, C.EINVAL, None) for n, d, *_ in C.corrupt()]
    for name, data, status, want in items:
        with open(os.path.join(out_dir, name + ".png"), "wb") as f:
            f.write(data)
        H, W = want.shape if want is not None else (70, 50)
        with open(os.path.join(out_dir, name + ".expect"), "wb") as f:
            f.write(b"%d %d %d\n" % (status, H, W))
            if want is not None:
                f.write(want.tobytes())
    print("%d files in %s" % (len(items), out_dir))


if __name__ == "__main__":
    main(sys.argv[1])
