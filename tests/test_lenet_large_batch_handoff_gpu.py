"""GPU test for the large-batch hand-off of the fused weight-grad + update
launchers: above B = 2048 hip_wgrad_update runs k_wgrad then k_update, and
hip_wgrad_update_momentum runs k_wgrad then k_update_mom, instead of the
single k_wgrad_update[_mom] launch.

B = 2049 is the smallest batch that takes the branch.  One train-mode
hip_fwdbwd (fp32 activations, seeded synthetic data) feeds both forms; each
form runs the fused binding (path A) and the same two kernels through
hip_wgrad_roles + hip_update[_momentum] (path B) on copies of one start
state.  A and B differ only in the order of the gradient atomics.

Agreement tolerance: 4x the A-vs-B max abs difference measured with this
test on the commit before the launchers took the optimizer as a value
(MI355X, three processes):
    plain     params 2.980e-08, 2.980e-08, 2.980e-08
    momentum  params 5.960e-08, 5.960e-08, 5.960e-08
    momentum  vel    1.788e-07, 2.980e-07, 2.384e-07
The largest of the three is the measured value.  The margin covers
atomic-order variation between runs; the results, 1.2e-7, 2.4e-7 and 1.2e-6,
stay far under the 1e-5 and 1e-5 / (1 - mu) bounds that
test_step_loop_and_graph_agree uses for the grid path.
"""
import pytest
import torch

from parallel_cnn_amd.ops import native
from parallel_cnn_amd.ops import shapes as S

pytestmark = pytest.mark.gpu

B = 2049
DT, SCALE = 0.1, 1.0 / B          # mean reduction, the trainer's default
MU, WD, NESTEROV = 0.9, 5e-4, True
ROLES = 7

PLAIN_P_TOL = 4 * 2.980e-08
MOM_P_TOL = 4 * 5.960e-08
MOM_V_TOL = 4 * 2.980e-07
assert PLAIN_P_TOL <= 1e-5 and max(MOM_P_TOL, MOM_V_TOL) <= 1e-5 / (1 - MU)


@pytest.fixture(scope="module")
def case(device):
    """One forward + backward-data at B = 2049; read-only for the tests."""
    C = native.require()
    gen = torch.Generator().manual_seed(2049)
    x = torch.rand(B, S.IN_PIX, generator=gen).to(device)
    labels = torch.randint(0, 10, (B,), generator=gen).to(device,
                                                          dtype=torch.int32)
    params = (0.5 - torch.rand(S.N_PARAMS, generator=gen)).to(device)
    vel = (0.01 * (0.5 - torch.rand(S.N_PARAMS, generator=gen))).to(device)
    a1 = torch.empty(B, S.C1_OUT, device=device)
    a2 = torch.empty(B, S.S1_OUT, device=device)
    y = torch.empty(B, S.FC_OUT, device=device)
    dz = torch.empty(B, S.FC_OUT, device=device)
    dz2 = torch.empty(B, S.S1_OUT, device=device)
    dz1 = torch.empty(B, S.C1_OUT, device=device)
    loss = torch.zeros(1, device=device)
    correct = torch.zeros(1, dtype=torch.int32, device=device)
    C.hip_fwdbwd(x, params, a1, a2, y, dz, dz2, dz1, labels, loss, correct,
                 B, 0, native.current_stream_handle())
    torch.cuda.synchronize()
    assert dz.abs().max().item() > 0
    return dict(acts=(x, a1, a2, dz, dz2, dz1), params=params, vel=vel)


def start_state(case):
    return (case["params"].clone(), torch.zeros_like(case["params"]),
            case["vel"].clone())


def check_pair(name, a, b, start, tol):
    diff = (a - b).abs().max().item()
    moved = (a - start).abs().max().item()
    print(f"{name}: A vs B max abs diff {diff:.3e} (tol {tol:.3e}), "
          f"moved {moved:.3e}")
    assert diff <= tol, (name, diff, tol)
    return moved


def test_momentum_handoff_matches_two_launches(case, device):
    C = native.require()
    sh = native.current_stream_handle()
    pa, ga, va = start_state(case)
    pb, gb, vb = start_state(case)
    ticket = torch.zeros(1, dtype=torch.int32, device=device)
    C.hip_wgrad_update_momentum(*case["acts"], ga, pa, va, DT, SCALE, MU, WD,
                                NESTEROV, ticket, B, 0, ROLES, sh)
    C.hip_wgrad_roles(*case["acts"], gb, B, 0, ROLES, sh)
    assert gb.abs().max().item() > 0
    C.hip_update_momentum(pb, gb, vb, DT, SCALE, MU, WD, NESTEROV, sh)
    torch.cuda.synchronize()
    moved = check_pair("momentum params", pa, pb, case["params"], MOM_P_TOL)
    check_pair("momentum vel", va, vb, case["vel"], MOM_V_TOL)
    assert moved > 100 * MOM_P_TOL, moved
    assert torch.count_nonzero(ga).item() == 0
    assert torch.count_nonzero(gb).item() == 0
    assert int(ticket.item()) == 0


def test_plain_handoff_matches_two_launches(case, device):
    C = native.require()
    sh = native.current_stream_handle()
    pa, ga, _ = start_state(case)
    pb, gb, _ = start_state(case)
    ticket = torch.zeros(1, dtype=torch.int32, device=device)
    C.hip_wgrad_update(*case["acts"], ga, pa, DT * SCALE, ticket, B, 0, ROLES,
                       sh)
    C.hip_wgrad_roles(*case["acts"], gb, B, 0, ROLES, sh)
    assert gb.abs().max().item() > 0
    C.hip_update(pb, gb, DT * SCALE, sh)
    torch.cuda.synchronize()
    moved = check_pair("plain params", pa, pb, case["params"], PLAIN_P_TOL)
    assert moved > 100 * PLAIN_P_TOL, moved
    assert torch.count_nonzero(ga).item() == 0
    assert torch.count_nonzero(gb).item() == 0
    assert int(ticket.item()) == 0
