"""The wave64 primitives have one home: bow_amd/csrc/wave_ops.h.  A DPP move (bound_ctrl, the row mask, what a lane without a source
receives), the one-wave LDS fence and the vector typedef of the 16-byte non-temporal loads are easy to get subtly wrong, and every
local copy is one more place a reviewer has to re-check - so no other device source may spell them."""
import glob
import os

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bow_amd", "csrc")
MARKERS = ["__builtin_amdgcn_update_dpp", "ext_vector_type", '"wavefront"']


def test_dpp_moves_wave_fences_and_vector_typedefs_live_in_wave_ops_h_only():
    sources = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert os.path.join(CSRC, "wave_ops.h") in sources and len(sources) > 30, "the device sources were not found"
    home = open(os.path.join(CSRC, "wave_ops.h")).read()
    for m in MARKERS:
        assert m in home, "%s is gone from wave_ops.h" % m
    found = {}
    for path in sources:
        if os.path.basename(path) == "wave_ops.h":
            continue
        text = open(path).read()
        hits = [m for m in MARKERS if m in text]
        if hits:
            found[os.path.basename(path)] = hits
    assert not found, "wave64 primitives spelled outside wave_ops.h (use its names): %s" % found
