"""The scenes, the dataset config and the sample parameters that tests/test_scene_prep_cpu.py and tests/test_scene_prep_gpu.py
share (built once per process, never modified).  Three ragged scenes:

  A  P = 6000, D = 7 (odd row length), K = 11 boxes against G = 8 (truncation); N = 5000 samples cross any tile many times
  B  P = 97,   D = 7, K = 5 boxes (three padding rows at -100 go through the transform); P < N: the choices repeat
  C  P = 1200, D = 135, K = 5 boxes, in a store of its own (D is per store)

Each scene is laid out around its sample (the choices are drawn first, the labels are placed with them in hand) to hold:
  id 0     a plain instance;  id 2047: the largest supported id
  id 5     spread over the whole index range (every 7th point), so every tile of the sample meets it
  id 9     an instance none of whose points is sampled: its table entry stays untouched, no NaN and no vote may come of it
  id 11    mixed semantic labels; its FIRST sampled point carries a voting label (so all of its sampled points vote)
  id 12    mixed semantic labels; its first sampled point carries a non-voting label (so none votes)
  id 13    a single point, sampled once (scenes A and C): its vote is 0
  ids 20.. plain instances, some with semantic ids outside nyu40ids (1, 2, 40)
Coordinates lie on both sides of zero, and every 11th point has an exact 0 in one coordinate."""
import numpy as np

NYU40IDS = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])
NYU40ID2CLASS = {int(v): i for i, v in enumerate(NYU40IDS)}
MEAN_SIZE_ARR = 0.3 + np.random.RandomState(7).rand(len(NYU40IDS), 3)     # (18, 3) fp64
G = 8
N_AB = 5000
N_C = 1024
_CACHE = {}


def _choices(rs, P, N, forced_in, forced_out):
    """N draws from [0, P) holding every index of forced_in and none of forced_out; without repeats when P >= N"""
    pool = np.setdiff1d(np.arange(P), np.concatenate([forced_in, forced_out]))
    if P >= N:
        rest = rs.permutation(pool)[:N - len(forced_in)]
    else:
        rest = rs.choice(pool, N - len(forced_in), replace=True)
    ch = np.concatenate([forced_in, rest])
    return ch[rs.permutation(N)].astype(np.int64)


def _scene(seed, P, D, K, N, single=True):
    rs = np.random.RandomState(seed)
    idx = np.arange(P)
    inst = 20 + (idx * 13 // max(P // 9, 1)) % 17                        # plain instances 20 .. 36 in runs
    sem = NYU40IDS[inst % len(NYU40IDS)].copy()
    sem[inst % 4 == 0] = np.array([1, 2, 40])[inst[inst % 4 == 0] % 3]   # some plain instances do not vote
    inst[idx % 7 == 0] = 5
    sem[idx % 7 == 0] = 5
    inst[1:30:2] = 0
    sem[1:30:2] = 4
    inst[P - 20:P - 4:3] = 2047
    sem[P - 20:P - 4:3] = 33
    unsampled = np.array([31, 32, 33, 34])
    inst[unsampled], sem[unsampled] = 9, 3
    mixed_a = np.array([37, 38, 39, 40, 41, 43, 44, 45])
    mixed_b = np.array([46, 47, 48, 50, 51, 52, 53, 54])
    inst[mixed_a], inst[mixed_b] = 11, 12
    forced_in = np.concatenate([[5], mixed_a[:3], mixed_b[:3]])          # (row 5 holds the signed zeros)
    if single:
        inst[57], sem[57] = 13, 6
        forced_in = np.append(forced_in, 57)
    choices = _choices(rs, P, N, forced_in, unsampled)
    # the first sampled point of 11 votes, the rest of 11 alternates; the first sampled point of 12 does not vote
    for ids, first_label, other in ((mixed_a, 3, 1), (mixed_b, 2, 7)):
        src = choices[np.isin(choices, ids)]                             # the instance's sampled points, in sample order
        sem[ids[0::2]], sem[ids[1::2]] = first_label, other
        sem[src[0]] = first_label
        sem[src[src != src[0]][0]] = other                               # both kinds stay present among the sampled points
    rows = rs.randn(P, D).astype(np.float32)
    rows[:, 0:3] *= np.array([4.0, 4.0, 1.5], dtype=np.float32)          # both signs
    rows[idx % 11 == 0, (idx[idx % 11 == 0] // 11) % 3] = 0.0            # exact zeros
    rows[5, 0:3] = [-0.0, 0.0, -0.0]
    boxes = np.zeros((K, 8))
    boxes[:, 0:3] = rs.uniform(-4, 4, (K, 3))
    boxes[:, 3:6] = rs.uniform(0.2, 2.5, (K, 3))
    boxes[:, 6] = NYU40IDS[rs.randint(0, len(NYU40IDS), K)]
    boxes[:, 7] = np.arange(K) + 3                                       # object ids 3 .. K + 2
    if K > 3:
        boxes[3, 7] = boxes[1, 7]                                        # one object id twice: the LAST match gives ref_*
    return dict(rows=rows, instance_labels=inst.astype(np.int64), semantic_labels=sem.astype(np.int64),
                instance_bboxes=boxes), choices


def _params(rs, choices, flips):
    """angles and translation from the reference's distributions (lib/dataset.py:467-483, 807-809)"""
    angles = [(rs.random_sample() * np.pi / 18) - np.pi / 36 for _ in range(3)]
    factor = [rs.choice(np.arange(-0.5, 0.501, 0.001), size=1)[0] for _ in range(3)]
    return dict(choices=choices, flip_x=flips[0], flip_y=flips[1], angles=angles, translation=factor)


def cases():
    """-> dict: scenes_ab [A, B], scenes_c [C], params_ab (2 dicts), params_c (1 dict), object_ids_ab, object_ids_c"""
    if not _CACHE:
        rs = np.random.RandomState(2024)
        a, ch_a = _scene(1, 6000, 7, 11, N_AB)
        b, ch_b = _scene(2, 97, 7, 5, N_AB, single=False)
        c, ch_c = _scene(3, 1200, 135, 5, N_C)
        _CACHE.update(scenes_ab=[a, b], scenes_c=[c],
                      params_ab=[_params(rs, ch_a, (-1, 1)), _params(rs, ch_b, (1, -1))],
                      params_c=[_params(rs, ch_c, (-1, -1))],
                      object_ids_ab=[4, -1], object_ids_c=[5])
    return _CACHE


def config():
    return dict(nyu40ids=NYU40IDS, nyu40id2class=NYU40ID2CLASS, mean_size_arr=MEAN_SIZE_ARR)


def check_layout(scene, choices):
    """the properties the docstring promises, asserted (a test calls this, so a change of the generator cannot lose them)"""
    inst, sem = scene["instance_labels"][choices], scene["semantic_labels"][choices]
    assert 0 in inst and 2047 in inst and 9 not in inst and 9 in scene["instance_labels"]
    j5 = np.nonzero(inst == 5)[0]
    assert j5.min() < 256 and j5.max() >= len(choices) - 256 and np.diff(j5).max() < 256      # every tile of 256 meets id 5
    f11, f12 = np.nonzero(inst == 11)[0][0], np.nonzero(inst == 12)[0][0]
    assert sem[f11] in NYU40IDS and sem[f12] not in NYU40IDS
    for i in (11, 12):
        labels = np.isin(sem[inst == i], NYU40IDS)
        assert labels.any() and not labels.all()                                              # mixed among the sampled points
    xyz = scene["rows"][choices, 0:3]
    assert (xyz < 0).any() and (xyz > 0).any() and (xyz == 0).any()
    assert not np.isin(sem, NYU40IDS).all()
