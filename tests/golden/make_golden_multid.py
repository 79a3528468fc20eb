"""Writes tests/golden/multid_generate.npz, the fixture of the Multi-dSprites generator (genesis_amd/generate_multid.py,
gx_sprites_compose).  The yardstick is the reference's own scripts/generate_multid.py, imported live, at zero tolerance: after
random.seed(0) it runs, in ONE random stream, every case of RUNS on the procedural sprite bank of tests/multid_bank.py:
    <run>_images   uint8 [N, 64, 64, 3]   the reference's float32 frames * 255 (asserted: u8.astype('float32') / 255.0 equals
                                          them bit for bit)
    <run>_masks    uint8 [N, 64, 64]      the reference's float64 instance masks
    <run>_choices  int64                  calls of random.choice the run made (RUNS records the expected number)
main() asserts what makes the fixture worth having: the recorded numbers of choice calls, colour redraws in the unique run, all
object counts 1..4 in the 48-image run, and an image in which a later sprite hides part of an earlier one.

Importing this module needs neither the reference nor the fixture; only main() does.
Run from the repository root: python tests/golden/make_golden_multid.py"""
import os
import os.path as osp
import random
import sys

import numpy as np

HERE = osp.dirname(osp.abspath(__file__))
NPZ = osp.join(HERE, 'multid_generate.npz')
REFERENCE_ROOT = os.environ.get('GENESIS_REFERENCE_ROOT', '/root/reference')

# (run, images, num_objects, unique, calls of random.choice)
RUNS = [('rand24', 24, None, False, 234), ('unique48', 48, None, True, 510), ('four8', 8, 4, False, 120)]
UNIQUE_REDRAWS = 4
SEED = 0


def import_reference_generator():
    import importlib.util
    spec = importlib.util.spec_from_file_location('ref_generate_multid', osp.join(REFERENCE_ROOT, 'scripts', 'generate_multid.py'))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    return ref


def main():
    sys.path.insert(0, osp.dirname(HERE))
    from multid_bank import SpriteBank
    ref = import_reference_generator()
    bank = SpriteBank()
    calls = {'choice': 0, 'randint': []}

    def counting_choice(seq):
        calls['choice'] += 1
        return random.choice(seq)

    def recording_randint(a, b):
        v = random.randint(a, b)
        calls['randint'].append((a, b, v))
        return v

    ref.choice, ref.randint = counting_choice, recording_randint
    random.seed(SEED)
    out = {}
    hidden = 0
    for name, n, num_objects, unique, want_choices in RUNS:
        calls['choice'], calls['randint'] = 0, []
        images, masks = ref.generate(bank, n, num_objects=num_objects, unique=unique)
        assert images.dtype == np.float32 and images.shape == (n, 64, 64, 3)
        assert masks.dtype == np.float64 and masks.shape == (n, 64, 64, 1)
        u8 = np.rint(images * 255.0).astype(np.uint8)
        assert np.array_equal(u8.astype('float32') / 255.0, images)
        m8 = masks[..., 0].astype(np.uint8)
        assert np.array_equal(m8.astype(np.float64), masks[..., 0])
        assert calls['choice'] == want_choices, (name, calls['choice'])
        sprites = [v for a, b, v in calls['randint'] if (a, b) == (0, 737279)]
        counts = [v for a, b, v in calls['randint'] if (a, b) == (1, 4)] if num_objects is None else [num_objects] * n
        assert len(counts) == n and sum(counts) == len(sprites)
        redraws = calls['choice'] // 3 - n - len(sprites)
        if name == 'unique48':
            assert redraws == UNIQUE_REDRAWS, redraws
            assert set(counts) == {1, 2, 3, 4}
        else:
            assert redraws == 0
        k = 0
        for i, c in enumerate(counts):                 # an earlier sprite with fewer visible pixels than it has
            for o in range(c):
                hidden += int((m8[i] == o + 1).sum()) < int(bank[sprites[k]].sum())
                k += 1
        out[name + '_images'], out[name + '_masks'] = u8, m8
        out[name + '_choices'] = np.int64(calls['choice'])
    assert hidden >= 1
    np.savez_compressed(NPZ, **out)
    print('%s: %d bytes, %d partly or wholly hidden sprites' % (NPZ, osp.getsize(NPZ), hidden))


if __name__ == '__main__':
    main()
