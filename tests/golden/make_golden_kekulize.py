"""Writes drd2_test.smi and drd2_valid.smi: the test and validation strings of the reference's DRD2 actives, copied byte
for byte as data, for tests/test_kekulize_cpu.py / test_kekulize_gpu.py to read with
``analyze.read_smiles(..., aromatic="kekulize")`` and its model.

    python tests/golden/make_golden_kekulize.py <reference checkout>/data/pre-training/DRD2_actives

Input: test.smi and valid.smi of that directory (data files without a header row: one "<string> <name>" row per
molecule, 432 + 431 rows).  The rules the tests read them under are written out in the tests: atom types C N O F S Cl
Br, formal charges -1 0 +1, implicit H 0-3, max_n_nodes 72.  The script asserts what the tests rely on — aromatic atoms
in all but 4 strings, no stereo mark, bracket atoms only from the list below, at most 68 atoms — and copies the files."""
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
BRACKETS = {"[nH]", "[n+]", "[s+]", "[O-]", "[N+]", "[S+]", "[CH2]", "[SH]"}


def main(src_dir):
    total = aromatic = 0
    brackets = set()
    for name, rows in (("test.smi", 432), ("valid.smi", 431)):
        with open(os.path.join(src_dir, name), "rb") as f:
            data = f.read()
        strings = [line.split(" ")[0] for line in data.decode("ascii").splitlines()]
        assert len(strings) == rows and strings[0] != "SMILES" and len(data) < 64 * 1024
        for s in strings:
            brackets.update(re.findall(r"\[[^\]]*\]", s))
            bare = re.sub(r"\[[^\]]*\]|Cl|Br", "", s)
            assert not re.search(r"[@/\\*$]", s) and not re.search(r"[ad-mq-rt-z]", bare), s
            assert len(re.findall(r"\[[^\]]*\]|Cl|Br|[A-Za-z]", s)) <= 68, s
            aromatic += bool(re.search(r"[bcnops]", re.sub(r"Cl|Br", "", s)))
        total += rows
        with open(os.path.join(HERE, "drd2_" + name), "wb") as f:
            f.write(data)
    assert brackets <= BRACKETS, brackets
    assert (total, aromatic) == (863, 859)
    print(f"{total} strings, {aromatic} with aromatic atoms, bracket atoms {sorted(brackets)}")


if __name__ == "__main__":
    main(sys.argv[1])
