"""CPU: the three numpy models of the kernels that share the labelled read (``gi_read_labelled`` of csrc/gi_molread.h)
agree on which molecules are malformed.  No device compute is issued.

``validity``'s verdict, ``fingerprint``'s zero row and ``smiles``' empty string are documented as agreeing on the low nine
status bits: the ``MALFORMED_BITS``, ``VAL_EMPTY`` = ``SMI_EMPTY`` and ``VAL_SELF_LOOP`` = ``SMI_SELF_LOOP``.  On the
device one function sets them for all three; here the same is asked of the models the device is held to
(tests/valence_model.py, fingerprint_model.py, smiles_model.py), on the hand-made molecules of test_valence_cpu.py: one
per malformed bit, the empty one, the self-bonded one, and three without any of the bits."""
from graphinvent_amd import analyze
from graphinvent_amd import lib as L
from tests import fingerprint_model as FM
from tests import smiles_model as SM
from tests import valence_model as VM
from tests.test_valence_cpu import model_rules, status_cases

LOW_NINE = 0x1FF


def test_the_three_models_set_the_same_low_nine_status_bits():
    assert L.VAL_EMPTY == L.SMI_EMPTY == 128 and L.VAL_SELF_LOOP == L.SMI_SELF_LOOP == 256
    assert analyze.MALFORMED_BITS | L.VAL_EMPTY | L.VAL_SELF_LOOP | L.MOL_OVERFLOW == LOW_NINE
    r, cases, seen = model_rules("gdb13"), status_cases(), 0
    for name, (nodes, edges, n, want) in cases.items():
        for given in (n, None) if name not in ("n_too_large", "onehot_none") else (n,):
            valence = int(VM.judge(nodes, edges, given, r)["status"]) & LOW_NINE
            fingerprint = int(FM.status_of(nodes, edges, given, r)[0])
            smiles = int(SM.write(nodes, edges, given, r)["status"]) & LOW_NINE
            assert valence == fingerprint == smiles == want & LOW_NINE, (name, given, valence, fingerprint, smiles)
            assert fingerprint & ~LOW_NINE == 0                               # the fingerprint has no other bits
            seen |= valence
    assert seen == LOW_NINE & ~L.MOL_OVERFLOW                                 # every bit had its molecule
    assert sum(1 for c in cases.values() if c[3] & LOW_NINE == 0) == 3       # sound, over, fragments
