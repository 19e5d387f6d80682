"""Golden fixtures of windowed inference on a gammatone model
(``tests/golden/gamma_windows.{json,npz}``): recorded results of the oracle
composition in ``tests/gamma_window_refs.py`` only (oracle/sed_oracle.py's own
functions, CPU, no library call) -- test infrastructure.

  gamma_windows.json   per case: preset, lengths, window spec, windows per clip, T and output
                       frames per window, merged frames per clip, the events of every clip's
                       averaged merge (and of the vote merge), the tie-guarded cell count (0) and
                       the distance of the framewise values from the thresholds (>= 1e-4)
  gamma_windows.npz    <case>_codes_<clip>_<window>   int16 [64, T] of each clip's first and last window
                       <case>_merged_<clip>           float32 [N, 25]
                       <case>_votes_<clip>            float32 [N, 25] (the main_strong case)

The tool asserts what the tests rely on: no cell of any window within the tie
guard of a rounding boundary, every framewise value at least 1e-4 from every
threshold applied to it.

Usage:  python tools/make_golden_gamma_windows.py
"""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'sound-event-detection_amd'), os.path.join(REPO, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import gamma_window_refs as W  # noqa: E402


def main():
    meta, arrays = {}, {}
    for name, c in W.CASES.items():
        guarded, dist = W.guarded_cells(name), W.threshold_distance(name)
        print('%-7s guarded cells %d, distance from the thresholds %.3g' % (name, guarded, dist))
        assert guarded == 0, (name, guarded)
        assert dist >= W.THRESHOLD_MARGIN, (name, dist)
        m = dict(preset=c.preset, seed=c.seed, lengths=list(c.lengths), sample_duration=c.sd, overlap_value=c.ov,
                 driver=c.driver, durations=W.durations(name), weight_seed=c.wseed, params=W.params(name), guarded=guarded, threshold_distance=dist,
                 n_windows=[], T=[], window_frames=[], merged_frames=[], events=W.events(name))
        for i in range(len(c.lengths)):
            o = W.clip_oracle(name, i)
            m['n_windows'].append(len(o.windows))
            m['T'].append([int(w.codes.shape[1]) for w in o.windows])
            m['window_frames'].append([int(w.framewise.shape[0]) for w in o.windows])
            m['merged_frames'].append(int(o.merged.shape[0]))
            for k in sorted({0, len(o.windows) - 1}):
                arrays['%s_codes_%d_%d' % (name, i, k)] = o.windows[k].codes
            arrays['%s_merged_%d' % (name, i)] = o.merged
            if o.votes is not None:
                arrays['%s_votes_%d' % (name, i)] = o.votes.astype(np.float32)
        if c.driver == 'main_strong':
            m['vote_events'] = W.vote_events(name)
        meta[name] = m
    gd = os.path.join(REPO, 'tests', 'golden')
    with open(os.path.join(gd, 'gamma_windows.json'), 'w') as f:
        json.dump(dict(cases=meta), f, indent=1, sort_keys=True)
        f.write('\n')
    np.savez_compressed(os.path.join(gd, 'gamma_windows.npz'), **arrays)
    print('wrote', sorted(arrays))


if __name__ == '__main__':
    main()
