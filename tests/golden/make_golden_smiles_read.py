"""Writes smiles_read_gdb13_1K.smi: the training strings of the reference's GDB-13 1K set, copied byte for byte as data,
for tests/test_smiles_read_cpu.py / test_smiles_read_gpu.py to read with ``analyze.read_smiles`` and its model.

    python tests/golden/make_golden_smiles_read.py <reference checkout>/data/pre-training/gdb13_1K

Input: train.smi of that directory (a data file: the header row "SMILES Name", then one "<string> <name>" row per
molecule).  The rules the tests read it under are that directory's preprocessing_params.csv values, written out in the
tests: atom types C N O S Cl, formal charges -1 0 +1, implicit H 0-3, max_n_nodes 13, no aromatic bonds.  The script
asserts what the reader's subset asks of the file — no aromatic lowercase atom, no stereo mark, no bracket atom other
than [N+] and [O-] — and copies it."""
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main(src_dir):
    with open(os.path.join(src_dir, "train.smi"), "rb") as f:
        data = f.read()
    lines = data.decode("ascii").splitlines()
    assert lines[0] == "SMILES Name" and len(lines) > 1
    strings = [line.split(" ")[0] for line in lines[1:]]
    brackets = set()
    for s in strings:
        brackets.update(re.findall(r"\[[^\]]*\]", s))
        bare = re.sub(r"\[[^\]]*\]|Cl|Br", "", s)
        assert not re.search(r"[a-z@/\\:*$]", bare), s
    assert brackets <= {"[N+]", "[O-]"}, brackets
    assert len(data) < 64 * 1024
    with open(os.path.join(HERE, "smiles_read_gdb13_1K.smi"), "wb") as f:
        f.write(data)
    print(f"{len(strings)} strings, {len(data)} bytes, bracket atoms {sorted(brackets)}")


if __name__ == "__main__":
    main(sys.argv[1])
