"""The pinned staging pair's THIRD piece, in both directions: the first piece whose buffer has been used before, so the first
that waits for the stream's use of it two pieces ago (inbound) or is handed over under a production into a buffer already
drained once (outbound).  No frames, no tracking: one volume of 256 x 256 x 272, whose linear form is 68 MiB -- with the 32 MiB
pinned buffers three plane batches of 128, 128 and 16 planes -- and whose image, every brick stored raw, has a payload of
34816 bricks x 2048 B = 68 MiB as well: three pieces of the unpack's upload behind the class table's one."""
import numpy as np
import pytest

import pack_twin as PT
from fuse_cases import make_ctx
from pack_cases import assert_same_image, ctx_fields

pytestmark = pytest.mark.gpu

DIMS = (256, 256, 272)
PIN_BYTES = 32 << 20


@pytest.fixture(scope="module")
def random_volume():
    """uniform-random int16 pairs (every brick of such a volume is RAW); read-only, shared by the tests"""
    x = np.random.default_rng(68).integers(-32768, 32768, (DIMS[2], DIMS[1], DIMS[0], 2), dtype=np.int16)
    assert x.nbytes > 2 * PIN_BYTES and x.nbytes // (DIMS[0] * DIMS[1] * 4) == 272
    x.setflags(write=False)
    return x


def test_upload_then_download_over_three_batches(hsk, random_volume):
    trk = make_ctx(hsk, DIMS, color=False)
    try:
        assert trk.stored_nz == DIMS[2]
        trk.upload_tsdf(random_volume)
        got = trk.download_tsdf()
        assert got.dtype == np.int16 and np.array_equal(got, random_volume)
    finally:
        trk.close()


def test_pack_and_unpack_a_payload_of_three_pieces(hsk, random_volume):
    trk = make_ctx(hsk, DIMS, color=False)
    other = make_ctx(hsk, DIMS, color=False)
    try:
        trk.upload_tsdf(random_volume)
        want = PT.pack(random_volume, None, ctx_fields(hsk, trk))
        info = PT.info(want)
        assert info["tsdf_bricks"][PT.RAW] == info["n_bricks"], info["tsdf_bricks"]
        assert info["tsdf_payload_bytes"] > 64 << 20       # more than two pinned buffers: a third piece, or this test checks nothing
        assert_same_image(trk.pack_volume(), want, "all-RAW volume")
        other.unpack_volume(want)
        assert np.array_equal(other.download_tsdf(), random_volume)
    finally:
        other.close()
        trk.close()
