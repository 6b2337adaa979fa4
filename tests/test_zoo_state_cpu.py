"""CPU: the drop-in contract of the model zoo (north_star: the product's modules stand behind the reference's model file,
model/pointnet2.py:5).  This package's five networks of that file, built with the same seed, against the state_dicts the
REFERENCE's own networks produce (tests/golden/g12_zoo_state.npz, tools/make_golden.py g12): keys in order, shapes, dtypes
and the seeded initial values (same registration order -> same draws).  The shipped checkpoint's side of the contract is
test_oracle_golden.py::test_checkpoint_state_contract_and_eval_golden."""
import torch

from conftest import golden
from test_oracle_golden import state_sha256

NETS = ["PointNet2ClsMsg", "PointNet2ClsSsg", "PointNet2PartSegSsg", "PointNet2PartSegMsg_one_hot", "PointNet2SemSeg"]


def test_product_network_state_dict_matches_the_reference():
    from pointnet12_amd import pointnet2 as M
    g = golden("g12_zoo_state.npz")
    for name in NETS:
        torch.manual_seed(0)
        net = getattr(M, name)(*[int(a) for a in g[name + "/args"]])
        sd = net.state_dict()
        assert list(sd) == [str(k) for k in g[name + "/keys"]], "%s: state_dict keys / order differ" % name
        assert ["x".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g[name + "/shapes"]], "%s: shapes differ" % name
        assert [str(v.dtype) for v in sd.values()] == [str(d) for d in g[name + "/dtypes"]], "%s: dtypes differ" % name
        assert state_sha256(net) == str(g[name + "/sha256"]), "%s: seeded initial values differ" % name
