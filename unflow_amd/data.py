"""Where each dataset's frames live under the data root (dirs.data of config.ini): what the inputs need of the reference's Data
classes (kitti/data.py, synthia/data.py, cityscapes/data.py, chairs/data.py) — `current_dir` and `get_raw_dirs()`.  No download,
no conversion, nothing on disk is ever moved or deleted.

    kitti       kitti_raw/<date>/<drive>/image_02/data and image_03/data
    synthia     synthia/<seq>/<seq>/RGB/Stereo_Left/<view>
    cityscapes  cs/leftImg8bit_sequence_trainvaltest/<split>/<city>
    chairs      flying_chairs/image

Deviation: every listing is sorted().  The reference takes os.listdir order, which depends on the file system, so its example
list — and with it the seeded shuffle — differs from machine to machine.  A missing directory raises RuntimeError naming it.

KITTI benchmark exclusion.  The KITTI 2012 / 2015 benchmark pairs are frames of the raw drives; the reference moves them and
their neighbours out of kitti_raw once, when it downloads the drives (kitti/data.py:13-61).  Here KITTIData(exclude_lists_dir=DIR)
reads every *.txt of DIR in the format of UnFlow's files/kitti_excludes,

    000000_10 2011_09_26_drive_0005_sync\\2011_09_26\\2011_09_26_drive_0005_sync\\image_00\\data\\0000000810.png

(only lines whose first word ends in _10 count), and list_frames() — which Input.raw_pairs asks instead of os.listdir when a data
object has it — leaves out, for the named drive, every frame whose number lies in [n - 10, n + 12), in image_02 and image_03
alike, BEFORE pairs are formed; Input's skipped_frames filter then drops the pair that would straddle the hole.  The drive
directory is <date>/<date>_drive_<nnnn>_extract, or ..._sync when that is the one present."""
import os

from .core.input import frame_name_to_num

EXCLUDE_BEFORE = 10      # frames in front of a benchmark frame that go with it
EXCLUDE_AFTER = 12       # first frame number behind it that stays (the pair's second frame + 10 neighbours)


def _subdirs(path):
    if not os.path.isdir(path):
        raise RuntimeError("data directory not found: %s" % path)
    return [os.path.join(path, name) for name in sorted(os.listdir(path))]


class Data:
    """The data root alone: enough for the inputs that read their files relative to current_dir (evaluation, fine-tuning)."""

    def __init__(self, root):
        self.current_dir = root

    def get_raw_dirs(self):
        return []


class KITTIData(Data):
    def __init__(self, root, exclude_lists_dir=None):
        super().__init__(root)
        self.excluded = read_kitti_excludes(exclude_lists_dir) if exclude_lists_dir else {}

    def get_raw_dirs(self):
        return [os.path.join(drive, view, 'data') for date in _subdirs(os.path.join(self.current_dir, 'kitti_raw'))
                for drive in _subdirs(date) for view in ('image_02', 'image_03')]

    def _holes(self, folder):
        """Frame numbers named by the exclude lists for the drive that `folder` (…/<date>/<drive>/image_0x/data) belongs to."""
        parts = os.path.normpath(folder).split(os.sep)
        if len(parts) < 4 or parts[-2] not in ('image_02', 'image_03'):
            return ()
        drive = parts[-3]
        for suffix in ('_extract', '_sync'):
            if drive.endswith(suffix):
                return self.excluded.get((parts[-4], drive[:-len(suffix)]), ())
        return ()

    def list_frames(self, folder):
        """The sorted listing of a raw directory without the benchmark frames and their neighbours."""
        listing = sorted(os.listdir(folder))
        holes = self._holes(folder)
        if not holes:
            return listing
        return [name for name in listing
                if not any(n - EXCLUDE_BEFORE <= frame_name_to_num(name) < n + EXCLUDE_AFTER for n in holes)]


class SynthiaData(Data):
    def get_raw_dirs(self):
        return [view for seq in _subdirs(os.path.join(self.current_dir, 'synthia'))
                for view in _subdirs(os.path.join(seq, os.path.basename(seq), 'RGB', 'Stereo_Left'))]


class CityscapesData(Data):
    def get_raw_dirs(self):
        top = os.path.join(self.current_dir, 'cs', 'leftImg8bit_sequence_trainvaltest')
        return [city for split in _subdirs(top) for city in _subdirs(split)]


class ChairsData(Data):
    def get_raw_dirs(self):
        folder = os.path.join(self.current_dir, 'flying_chairs', 'image')
        if not os.path.isdir(folder):
            raise RuntimeError("data directory not found: %s" % folder)
        return [folder]


def read_kitti_excludes(lists_dir):
    """{(date, '<date>_drive_<nnnn>'): sorted frame numbers} from every *.txt of lists_dir; lines whose first word does not end
    in _10 (the _11 frames are the pairs' second frames, covered by the window) and lines that name no drive are skipped."""
    if not os.path.isdir(lists_dir):
        raise RuntimeError("KITTI exclude lists not found: %s" % lists_dir)
    found = {}
    for name in sorted(os.listdir(lists_dir)):
        if not name.endswith('.txt'):
            continue
        with open(os.path.join(lists_dir, name)) as f:
            for line in f:
                words = line.split()
                if len(words) < 2 or not words[0].endswith('_10'):
                    continue
                path = words[-1].replace('\\', '/').split('/')
                if '_drive_' not in path[0]:
                    continue
                date, rest = path[0].split('_drive_', 1)
                drive = '%s_drive_%s' % (date, rest.split('_')[0])
                found.setdefault((date, drive), set()).add(frame_name_to_num(path[-1]))
    return {k: sorted(v) for k, v in found.items()}
