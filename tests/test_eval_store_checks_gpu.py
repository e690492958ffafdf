"""The device-side store checks of the evaluation kernels (csrc/eval_common.h, used by csrc/moteval.hip, csrc/hota.hip and
csrc/evalprep.hip): a device copy of the store that disagrees with the host's is flagged, never indexed by.

Two sequences of 6 frames and 3 objects.  After the evaluator is built ONE value of the device copy of sequence 0 is overwritten
(the host copy of the sequence table stays right, so the call reaches the kernels); sequence 1 stays intact and lies behind
sequence 0 in every array, so every planted value still indexes inside the store's and the workspace's allocations: a lost
check shows as a wrong flag word, never as a fault.  The flag words and the messages are literals recorded from the commit
before the checks were merged into one header.

    case 1   seq[0].n_gt = st.n_gt + 1                       the slice check fails before anything is indexed
    case 2   det_perm[k] = n_det of sequence 0               k: the first row of frame F
    case 3   gt_off[F + 1] = gt_off[F] - 1                   of sequence 0
    case 4   gt_id[i] = n_obj of sequence 0                  i: the first GT row of frame F (MOT and HOTA only)

HOTA counts the rows of every object over the whole sequence before it walks the frames, so it meets the id of case 4 there
and names no frame; the MOT walk meets it in frame F."""
import numpy as np
import pytest

from tests.test_evalprep_gpu import same
from trackmpnn_amd.evalprep import KITTI_CAR, EvalPrep, evalprep_host, synth_prep_sequence
from trackmpnn_amd.hota import HotaEvaluator, hota_host
from trackmpnn_amd.moteval import MotEvaluator, mot_events_host, mot_summary_host, synth_mot_sequence

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T0, F = 5, 3                   # first frame of sequence 0; the (middle, non-empty) frame the faults are planted in
AT_F = 4 | (F + 1) << 8         # = 1028: FLAG_STORE, and frame F + 1 counted from 1
MOT_TEXT = 'the store is inconsistent (an offset, a permutation entry or an object id out of range)'
PREP_TEXT = 'the store is inconsistent (an offset or a permutation entry out of range)'
#                 case:   1      2      3      4
FLAGS = {'mot':   (None, 4,     4,     1028,  1028),
         'ident': (None, 4,     4,     1028,  1028),
         'hota':  (None, 4,     4,     1028,  4),
         'prep':  (None, 4,     1028,  1028)}
WHO = {'mot': 'MotEvaluator', 'ident': 'MotEvaluator', 'hota': 'HotaEvaluator', 'prep': 'EvalPrep'}
ARGS = ('det_frame', 'det_box', 'tracks', 'gt_frame', 'gt_track', 'gt_box')


@pytest.fixture(scope='module')
def sets():
    """The two sets and the host definitions of sequence 1, computed once and left unchanged."""
    exact = dict(objects=3, p_absent=0.0, p_miss=0.0)
    mot = [synth_mot_sequence(11, 6, p_untracked=0.0, t0=T0, **exact), synth_mot_sequence(12, 6, **exact)]
    prep = [synth_prep_sequence(11, 6, t0=T0, **exact), synth_prep_sequence(12, 6, **exact)]
    a = [mot[1][k] for k in ARGS]
    ref = {'mot': mot_events_host(*a), 'ident': mot_summary_host(*a), 'hota': hota_host(*a),
           'prep': evalprep_host(prep[1], prep[1]['tracks'], KITTI_CAR)}
    return mot, prep, ref


def build(kind, mot, prep):
    if kind == 'prep':
        return EvalPrep(prep, KITTI_CAR, DEV)
    return HotaEvaluator(mot, DEV) if kind == 'hota' else MotEvaluator(mot, DEV, identity=kind == 'ident')


def plant(ev, case):
    """One wrong value in the device copy of sequence 0 (whose bases are all 0)."""
    st, t = ev.store, ev._t
    n_gt0, n_det0, n_frames0 = (int(v) for v in (st.seq[0, 1], st.seq[0, 3], st.seq[0, 5]))
    assert st.S == 2 and n_frames0 == 6 and not st.seq[0, [0, 2, 4, 6]].any()
    g0, g1, d0, d1 = (int(v) for v in (st.gt_off[F], st.gt_off[F + 1], st.det_off[F], st.det_off[F + 1]))
    assert 1 <= g0 < g1 <= n_gt0 and 0 <= d0 < d1 <= n_det0       # frame F is non-empty on both sides, rows before it
    assert st.seq[1, 1] > 0 and st.seq[1, 3] > 0                  # sequence 1 lies behind every planted index
    if case == 1:
        t['seq'][0, 1] = st.n_gt + 1
    elif case == 2:
        t['det_perm'][d0] = n_det0
    elif case == 3:
        t['gt_off'][F + 1] = g0 - 1
    else:
        assert st.seq[1, 7] > 0
        t['gt_id'][g0] = int(st.seq[0, 7])


def run(ev, kind, mot, prep):
    if kind == 'prep':
        ev.apply([q['tracks'] for q in prep])
    else:
        ev.evaluate([q['tracks'] for q in mot])


@pytest.mark.parametrize('kind,case', [(k, c) for k in ('mot', 'ident', 'hota', 'prep') for c in range(1, len(FLAGS[k]))])
def test_a_wrong_device_store_is_flagged_not_indexed(sets, kind, case):
    mot, prep, ref = sets
    ev = build(kind, mot, prep)
    plant(ev, case)
    run(ev, kind, mot, prep)
    per, _ = ev.read(check=False)
    print(f'{kind} case {case}: flag words {per[0]["flag"]}, {per[1]["flag"]}')
    want = FLAGS[kind][case]
    assert per[0]['flag'] == want
    assert per[1].pop('flag') == 0
    if kind == 'prep':
        assert per[1] == ref['prep'][2]
        assert np.array_equal(ev.filtered_tracks()[1].cpu().numpy(), ref['prep'][0])
    else:
        assert same(per[1], ref[kind])
    text = PREP_TEXT if kind == 'prep' else MOT_TEXT
    msg = f'{WHO[kind]}.read: sequence 0' + (f', frame {T0 + F}: ' if want == AT_F else ': ') + text
    with pytest.raises(RuntimeError) as e:
        ev.read()
    assert str(e.value) == msg
