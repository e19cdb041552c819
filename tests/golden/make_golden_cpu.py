"""Fixtures that let the CPU tests run without a reference checkout, produced from the UNMODIFIED reference
(``GI_REFERENCE_DIR`` = a reference checkout's graphinvent/ directory, its data/ directory beside it):

  gdb13_1K-debug_train.h5, gdb13_1K-debug_valid.h5
                          the reference's shipped preprocessed files (data/pre-training/gdb13_1K-debug/), byte for byte:
                          what tests/test_loader_cpu.py reads through libhdf5 and compares with the .npz copies.
  golden_constructor.npz  SHA-256 of every tensor of the reference ``GGNN`` / ``AttentionGGNN`` state_dict constructed
                          after ``torch.manual_seed(123)`` with the GDB-13 defaults (tests/test_boundary_cpu.py: the
                          drop-in constructors must consume the RNG identically; 12.5 M floats, so digests, not values).
  golden_callers_cpu.npz  the UNMODIFIED ``Workflow`` training path (3 epochs, whole-file batches) and
                          ``GraphGenerator.build_graphs`` (draws pinned) on ``ref_callers.cpu_model_modules()`` — a CPU
                          model and the drop-in loader from this repository — so that tests/test_callers_cpu.py can hold
                          the restated callers (oracle/callers_oracle.py) to them bit for bit.  Checked before it is
                          written: the restated callers reproduce it in this process.

Both runs pin ``torch.set_num_threads(1)`` (as the test does) so that CPU GEMM summation order cannot depend on the box.
    python tests/golden/make_golden_cpu.py"""
import hashlib
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import callers_oracle as CO            # noqa: E402
from oracle import ggnn_oracle as O                # noqa: E402
from tests.golden import ref_callers as RC         # noqa: E402

DATA = os.path.join(os.path.dirname(RC.REF), "data", "pre-training", "gdb13_1K-debug")
# the model and run of tests/test_callers_cpu.py
SMALL = dict(hidden_node_features=24, message_size=24, enn_hidden_dim=32, gather_width=24, gather_att_hidden_dim=32,
             gather_emb_hidden_dim=32, mlp1_hidden_dim=48, mlp2_hidden_dim=48)
SEED, EPOCHS, BATCH, LR, GEN_BATCH, DRAW_SEED = 3, 3, 100, 1e-3, 24, 0


def tensor_digest(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().contiguous().numpy().tobytes()).hexdigest()


def constructor_digests() -> dict:
    for m in [k for k in sys.modules if k == "gnn" or k.startswith("gnn.")]:
        del sys.modules[m]
    sys.path.insert(0, RC.REF)
    try:
        import gnn.mpnn as ref_mpnn
    finally:
        sys.path.remove(RC.REF)
    assert ref_mpnn.__file__.startswith(RC.REF)
    c = O.as_constants(O.make_config())
    out = {}
    for name in ("GGNN", "AttentionGGNN"):
        torch.manual_seed(123)
        sd = getattr(ref_mpnn, name)(c).state_dict()
        out[f"{name}::keys"] = np.array(list(sd))
        out[f"{name}::sha256"] = np.array([tensor_digest(v) for v in sd.values()])
    for m in [k for k in sys.modules if k == "gnn" or k.startswith("gnn.")]:
        del sys.modules[m]
    return out


def callers_run(make_workflow, make_generator, consts) -> dict:
    torch.manual_seed(SEED)
    wf = make_workflow(consts)
    wf.train_dataloader = wf.get_dataloader(wf.train_h5_path, "training set")
    wf.valid_dataloader = wf.get_dataloader(wf.valid_h5_path, "validation set")
    start, end = wf.define_model_and_optimizer()
    losses = []
    for epoch in range(start, end):
        wf.current_epoch = epoch
        losses.append((float(wf.train_epoch()), float(wf.validation_epoch())))
    draw = CO.InverseCdfDraws(DRAW_SEED, GEN_BATCH)
    RC.pin_multinomial(draw)
    with torch.no_grad():
        gen = make_generator(wf.model.eval(), GEN_BATCH, draw)
        n = gen.build_graphs()
    out = {"losses": np.array(losses), "n_generated": np.array(n), "rounds": np.array(draw.round),
           "nodes": gen.generated_nodes.numpy(), "edges": gen.generated_edges.numpy(),
           "n_nodes": gen.generated_n_nodes.numpy(), "likelihoods": gen.generated_likelihoods.numpy(),
           "terminated": gen.properly_terminated.numpy()}
    out.update({"final::" + k: v.detach().numpy().copy() for k, v in wf.model.state_dict().items()})
    return out


def main():
    assert RC.have_reference(), f"no reference checkout at {RC.REF}"
    for split in ("train", "valid"):
        shutil.copyfile(os.path.join(DATA, f"{split}.h5"), os.path.join(HERE, f"gdb13_1K-debug_{split}.h5"))
    np.savez_compressed(os.path.join(HERE, "golden_constructor.npz"), **constructor_digests())

    data_dir = tempfile.mkdtemp(prefix="gi_callers_cpu_")
    for name in ("train", "valid", "test"):
        shutil.copyfile(os.path.join(DATA, "valid.h5"), os.path.join(data_dir, f"{name}.h5"))
    consts = RC.as_constants(dict(RC.constants_dict("cpu", O.make_config(**SMALL), data_dir, batch_size=BATCH,
                                                    epochs=EPOCHS), init_lr=LR))
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        with RC.isolated():
            WF, GG = RC.load("cpu", consts)
            ref = callers_run(lambda c: WF.Workflow(constants=c),
                              lambda m, b, draw: GG.GraphGenerator(model=m, batch_size=b), consts)
        with RC.isolated():
            RC.cpu_model_modules()
            mine = callers_run(CO.WorkflowOracle, lambda m, b, draw: CO.GeneratorOracle(m, b, consts, draw), consts)
    finally:
        torch.set_num_threads(threads)
    shutil.rmtree(data_dir)
    assert set(ref) == set(mine) and all(np.array_equal(ref[k], mine[k]) for k in ref), \
        [k for k in ref if not np.array_equal(ref[k], mine[k])]
    assert int(ref["n_generated"]) > 0
    np.savez_compressed(os.path.join(HERE, "golden_callers_cpu.npz"), **ref)
    print("losses", ref["losses"].tolist(), "generated", int(ref["n_generated"]), "rounds", int(ref["rounds"]))


if __name__ == "__main__":
    main()
