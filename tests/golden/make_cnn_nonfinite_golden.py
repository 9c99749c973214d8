"""Generate tests/golden/nonfinite_<config>.npz for the 12 cnn fixtures: the REFERENCE's eval
forward on the ten-clip batch of tests/cnn_nonfinite_cases.py -- single NaN / -NaN / +Inf / -Inf
entries the model reads, and NaN / +Inf / -Inf fills of the entries it never reads.

The dead rows and columns are found with the reference itself: the fixture's first clip with NaN
in one whole row or one whole column per probe clip; the row or column is dead if the logits of
its clip hold no NaN.  The file holds the base fixture's name, the poke list, the dead lists, the
reference's logits and a CRC32 of the batch, which the tests rebuild from the base fixture
(cnn_nonfinite_cases.batch).  Fails unless the reference's logits are NaN in every logit of clips
1-4 and 9, finite in clips 0 and 5, and bit-equal in clips 6-8 to the same batch without the
fills.  Runs only in the build container (imports the reference with make_golden's stubs).

Usage:  python tests/golden/make_cnn_nonfinite_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)
import cnn_nonfinite_cases as nf  # noqa: E402
from golden_util import load_fixture  # noqa: E402
from make_golden import _stub_imports  # noqa: E402


def main():
    _stub_imports()
    import utils.model as mod  # the reference
    torch.set_num_threads(8)
    for name in nf.NAMES:
        cfg, params, x0, _, meta = load_fixture(name)
        model = mod.find_model(meta["model"])(cfg)
        model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
        model.eval()

        def run(x):
            with torch.no_grad():
                return model(torch.from_numpy(x)).numpy()

        H, W = x0.shape[1:]
        dead_rows, dead_cols = nf.dead_from_logits(np.concatenate([run(xb) for xb in nf.probe_batches(x0[0])]), H, W)
        x, pk = nf.batch(x0, dead_rows, dead_cols)
        logits = run(x)
        nofill = run(nf.batch(x0, dead_rows, dead_cols, fills=False)[0])
        assert np.isnan(logits[list(nf.LIVE_CLIPS)]).all(), (name, nf.pattern(logits))
        assert np.isfinite(logits[list(nf.CLEAN_CLIPS)]).all(), (name, nf.pattern(logits))
        fills = list(nf.FILL_CLIPS)
        assert np.array_equal(logits[fills], nofill[fills]) and np.isfinite(nofill[fills]).all(), name
        np.savez_compressed(os.path.join(HERE, f"nonfinite_{name}.npz"), fixture=np.array(name),
                            pokes=np.array(pk, dtype=np.int32), dead_rows=np.array(dead_rows, dtype=np.int32),
                            dead_cols=np.array(dead_cols, dtype=np.int32), logits=logits.astype(np.float32),
                            crc=np.array(nf.crc(x), dtype=np.uint32))
        print(f"{name:22s} dead rows {dead_rows} columns {dead_cols} {nf.pattern(logits)}")


if __name__ == "__main__":
    main()
