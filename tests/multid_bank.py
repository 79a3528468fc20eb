"""A procedural stand-in for the dSprites archive (737 280 binary 64 x 64 sprites, 3 GB unpacked), for the Multi-dSprites
generator's tests and fixture: the same length and the same item type, every sprite a function of its index.  A helper, not a
test.

With h = (i * 2654435761) & 0xffffffff, sprite i is centred at (8 + (h >> 4) % 48, 8 + (h >> 12) % 48) (x, y), has half-axes
(3 + (h >> 20) % 14, 3 + (h >> 25) % 14), and is a filled ellipse when h & 1, else a filled rectangle; set pixels are 1."""
import numpy as np

NUM_SPRITES = 737280
SIZE = 64


class SpriteBank(object):
    def __len__(self):
        return NUM_SPRITES

    def __getitem__(self, i):
        i = int(i)
        if not 0 <= i < NUM_SPRITES:
            raise IndexError(i)
        h = (i * 2654435761) & 0xffffffff
        cx, cy = 8 + (h >> 4) % 48, 8 + (h >> 12) % 48
        ax, ay = 3 + (h >> 20) % 14, 3 + (h >> 25) % 14
        y, x = np.mgrid[0:SIZE, 0:SIZE]
        dx, dy = x - cx, y - cy
        if h & 1:
            inside = dx * dx * (ay * ay) + dy * dy * (ax * ax) <= ax * ax * ay * ay
        else:
            inside = (np.abs(dx) <= ax) & (np.abs(dy) <= ay)
        return inside.astype(np.uint8)


def first_sprites(n):
    """uint8 [n, 64, 64]: the bank's first n sprites as one array (what an archive's 'imgs' holds)."""
    bank = SpriteBank()
    return np.stack([bank[i] for i in range(n)])
