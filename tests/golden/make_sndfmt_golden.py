"""Regenerates sndfmt_vectors.npz from CPython's `audioop` (present up to Python 3.12): the outside reference for the G.711
tables and the IMA ADPCM step of inaspeechsegmenter_amd/sndfmt.py and csrc/adpcm.hip.  The tests read the .npz only.

    python tests/golden/make_sndfmt_golden.py

ulaw, alaw: the 256 decoded values.  ima_nibbles[k] (200 nibbles in stream order), ima_pred[k], ima_index[k]: a random stream
and start state; ima_out[k]: the 200 samples audioop.adpcm2lin decodes from them.  audioop reads the HIGH nibble of a byte
first, WAV stores the low nibble first: the stream order is kept here by packing nibble 2i into the high half for audioop."""
import audioop
import os

import numpy as np

STREAMS, NIBBLES = 128, 200


def main():
    ulaw = np.frombuffer(audioop.ulaw2lin(bytes(range(256)), 2), dtype='<i2')
    alaw = np.frombuffer(audioop.alaw2lin(bytes(range(256)), 2), dtype='<i2')
    rng = np.random.default_rng(20261016)
    nib = rng.integers(0, 16, (STREAMS, NIBBLES), dtype=np.uint8)
    nib[: STREAMS // 4] |= rng.integers(0, 2, (STREAMS // 4, NIBBLES), dtype=np.uint8) * 4      # some that climb the step table
    pred = rng.integers(-32768, 32768, STREAMS).astype(np.int16)
    index = rng.integers(0, 89, STREAMS).astype(np.uint8)
    pred[:4] = (-32768, 32767, 0, -1)
    index[:4] = (88, 88, 0, 0)
    out = np.zeros((STREAMS, NIBBLES), dtype=np.int16)
    for k in range(STREAMS):
        packed = ((nib[k, 0::2] << 4) | nib[k, 1::2]).astype(np.uint8).tobytes()
        pcm, _ = audioop.adpcm2lin(packed, 2, (int(pred[k]), int(index[k])))
        out[k] = np.frombuffer(pcm, dtype='<i2')
    here = os.path.dirname(os.path.abspath(__file__))
    np.savez_compressed(os.path.join(here, 'sndfmt_vectors.npz'), ulaw=ulaw, alaw=alaw, ima_nibbles=nib, ima_pred=pred,
                        ima_index=index, ima_out=out)


if __name__ == '__main__':
    main()
