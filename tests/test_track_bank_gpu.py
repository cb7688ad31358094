"""GPU: the two track-bank kernels (clipops_bank_update_f32, clipops_bank_result_rows_f32, memotr_amd/csrc/clip_tracks.h)
against their host statements (memotr_amd/functions/clip_ops.py: bank_update_reference on the same device tensors --
torch's sigmoid there is the kernel's 1 / (1 + expf(-x)) -- and bank_result_rows_reference on the CPU, whose float32
arithmetic is exact), bit for bit: one and three streams, detect-row counts around the 64-lane and 256-thread edges, banks
of 16, 64 and 208 slots with holes in alternating slots, all free and none free, strided model outputs, guard words past
every table, the same bits from two launches, and several frames in a row."""
import pytest
import torch

from test_track_bank_cpu import DET_T, MISS, TRACK_T, assert_banks_equal, clone_bank, random_bank, random_outputs

from memotr_amd.functions import clip_ops
from memotr_amd.models.track_bank import ROW_FIELDS, TrackBank
from memotr_amd.results import BankResultLog

pytestmark = pytest.mark.gpu

N_DET = (1, 63, 64, 65, 300)
CAPS = (16, 64, 208)
PATTERNS = ("alternating", "none", "all")          # which slots hold a track: every other one, none, all
SHAPES = [(1, 8, True), (8, 256, False), (3, 100, True)]       # K, C, use_dab
GUARD = 64
STREAM_FIELDS = ROW_FIELDS + ("next_id", "counters", "free_list")


def guarded(t, value):
    """``t`` as the head of a larger buffer whose tail holds ``value``: (the view, the tail)."""
    buf = torch.full((t.numel() + GUARD,), value, dtype=t.dtype, device=t.device)
    buf[:t.numel()] = t.reshape(-1)
    return buf[:t.numel()].view(t.shape), buf[t.numel():]


def guard_bank(bank):
    tails = {}
    for name in STREAM_FIELDS:
        t = getattr(bank, name)
        view, tails[name] = guarded(t, -77 if not t.is_floating_point() else -7.5)
        setattr(bank, name, view)
    return tails


def assert_guards(tails):
    for name, tail in tails.items():
        assert (tail == (-77 if not tail.is_floating_point() else -7.5)).all(), name


@pytest.mark.parametrize("K,C,use_dab", SHAPES)
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("B", [1, 3])
def test_the_update_kernel_equals_the_host_statement(clip_lib, B, pattern, K, C, use_dab):
    born = dropped = retired = 0
    for n_det in N_DET:
        for cap in CAPS:
            seed = 1000 * n_det + cap + K
            res = random_outputs(B, n_det, cap, K, seed, use_dab=use_dab, C=C, device="cuda", strided=n_det % 2 == 1,
                                 birth_rate=0.8 if n_det == 65 else 0.2)
            start = random_bank(B, cap, K, seed, pattern=pattern, use_dab=use_dab, C=C, device="cuda")
            want, got, again = clone_bank(start), clone_bank(start), clone_bank(start)
            clip_ops.bank_update_reference(res, want, DET_T, TRACK_T, MISS)
            tails = guard_bank(got)
            clip_ops.bank_update(res, got, DET_T, TRACK_T, MISS)
            clip_ops.bank_update(res, again, DET_T, TRACK_T, MISS)
            assert_banks_equal(want, got)
            assert_banks_equal(got, again)                  # two launches, the same bits
            assert_guards(tails)
            live0, live1 = int((start.ids >= 0).sum()), want.counters[:, 0].sum().item()
            placed = int((want.next_id - start.next_id).sum())
            born, dropped = born + placed, dropped + int(want.counters[:, 1].sum())
            retired += live0 + placed - live1
            free = got.ids < 0
            for name in ROW_FIELDS[1:]:
                assert not getattr(got, name)[free].any(), (name, n_det, cap)
    if pattern != "all":
        assert born > 50
    if pattern != "none":
        assert retired > 20
    assert dropped > 0


def test_frames_in_a_row_keep_kernel_and_host_statement_equal(clip_lib):
    """Slots freed by one frame are refilled by the next; the two banks never part."""
    B, n_det, cap, K, C = 3, 65, 48, 8, 256
    want = TrackBank(B, cap, num_classes=K, hidden_dim=C, use_dab=False, device="cuda")
    got = clone_bank(want)
    reused = 0
    for frame in range(6):
        res = random_outputs(B, n_det, cap, K, seed=frame, use_dab=False, C=C, device="cuda", birth_rate=0.2)
        res["pred_logits"][:, :n_det] -= 2.5                 # fewer births per frame: the bank fills slowly
        holes = want.ids < 0
        clip_ops.bank_update_reference(res, want, DET_T, TRACK_T, MISS)
        clip_ops.bank_update(res, got, DET_T, TRACK_T, MISS)
        assert_banks_equal(want, got)
        if frame:
            reused += int(((want.ids >= 0) & holes).sum())
    assert reused > 0 and int(want.next_id.min()) > 5 and (want.ids < 0).any()
    got.check()


@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("B", [1, 3])
def test_the_result_row_kernel_equals_the_host_statement(clip_lib, B, K):
    sizes = [(1080, 1920), (480, 641), (97, 131)][:B]
    for cap in CAPS:
        for pattern in PATTERNS:
            host_bank = random_bank(B, cap, K, seed=cap + K, pattern=pattern, C=8)
            live = (host_bank.ids >= 0)[..., None]
            host_bank.boxes.copy_(host_bank.boxes.sigmoid() * 0.5 * live)
            host_bank.scores.copy_(host_bank.logits.sigmoid() * live)
            dev_bank = random_bank(B, cap, K, seed=cap + K, pattern=pattern, C=8, device="cuda")
            dev_bank.boxes, dev_bank.scores = host_bank.boxes.cuda(), host_bank.scores.cuda()
            host, dev = BankResultLog("cpu", capacity=8), BankResultLog("cuda", capacity=8)
            for frame in range(2):
                seq_frame = torch.tensor([[3 + b, frame] for b in range(B)])
                ori_wh = torch.tensor([[w, h] for h, w in sizes], dtype=torch.float32)
                host.append(host_bank, seq_frame, ori_wh, 0.6, 100)
                dev.append(dev_bank, seq_frame.cuda(), ori_wh.cuda(), 0.6, 100)
            counters = dev.counters.cpu()
            assert counters.tolist() == host.counters.tolist() and counters[1] == 0
            m = int(counters[0])
            assert (m == 0) == (pattern == "none")
            assert torch.equal(dev.rows_f[:m].cpu().view(torch.int32), host.rows_f[:m].view(torch.int32))
            assert torch.equal(dev.rows_i[:m].cpu(), host.rows_i[:m])
            assert sorted(dev.read()) == sorted(host.read())
            # the capacity rule, with guard words behind every table
            capacity = max(m // 2 - 1, 0)
            rows_f, tail_f = guarded(torch.zeros(capacity, 5, device="cuda"), -7.5)
            rows_i, tail_i = guarded(torch.zeros(capacity, 4, dtype=torch.int64, device="cuda"), -77)
            cnt, tail_c = guarded(torch.zeros(2, dtype=torch.int32, device="cuda"), -77)
            clip_ops.bank_result_rows(dev_bank, seq_frame.cuda(), ori_wh.cuda(), 0.6, 100, rows_f, rows_i, cnt)
            stored = min(capacity, m // 2)
            assert cnt.tolist() == [stored, m // 2 - stored]
            assert torch.equal(rows_f[:stored].cpu().view(torch.int32), host.rows_f[m // 2:m // 2 + stored].view(torch.int32))
            assert (tail_f == -7.5).all() and (tail_i == -77).all() and (tail_c == -77).all()
