"""Every HIP resource of the host layer belongs to an owner that frees it when its struct goes (csrc/srcnn_owned.hpp).  The
other GPU tests reach the lanes, the trimmed staging and the frozen stream graphs; this one takes the remaining owners --
stream workspaces, frame-stream slots with and without their graphs, a batch graph, the bounce slots, the host-call buffers,
the node lanes of two contexts, the stage timers' event pool -- through srcnn_shutdown three times over.  Valid calls only;
every result is the oracle's, bit for bit, in every cycle."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bit_equal
from libsrcnn_amd import synth

pytestmark = pytest.mark.gpu


def test_every_owner_survives_shutdown_init_and_trim(srcnn, oracle_lib):
    S, L = srcnn, srcnn.lib()
    y = synth.plane(33, 47, synth.SEED0 + 71, "noise")                 # h x w as numpy has it
    frames = synth.frames(5, 24, 40, 72, "noise")                       # five 40 x 24 frames
    tall = synth.plane(64, 48, synth.SEED0 + 73, "smooth")             # 128 output rows: one 64-row band per context
    img = np.random.default_rng(71).integers(0, 256, (70, 90, 4), dtype=np.uint8)
    want_y, want_tall = oracle_lib.y_path(y), oracle_lib.y_path(tall)
    want_frames = np.stack([oracle_lib.y_path(f) for f in frames])
    want_rgb, want_conv = oracle_lib.process(img, 2.0)

    def on_a_fresh_stream(what):
        h, w = y.shape
        din, dout = S.DeviceBuffer.from_numpy(y), S.DeviceBuffer(y.nbytes * 4)
        st = S.Stream()
        try:
            S.check(L.srcnn_y_upscale2x_f32_dev(din.ptr, w, h, dout.ptr, st.handle))
            st.sync()
        finally:
            st.destroy()                                               # and with it the stream's workspace
        assert_bit_equal(dout.to_numpy(np.float32, (2 * h, 2 * w)), want_y, what)
        din.free(); dout.free()

    try:
        for k in range(3):
            S.shutdown()
            assert S.init_devices([0, 0]) == 2
            on_a_fresh_stream("stream call, cycle %d" % k)

            # frame stream: slots, their copy streams and events; a slot captures a graph on its second frame, the eager call retires it
            assert_bit_equal(S.y_upscale2x_stream(frames, use_graph=True), want_frames, "graph stream, cycle %d" % k)
            assert S.stream_mode()[0] > 0, "no frame was replayed from a graph"
            assert_bit_equal(S.y_upscale2x_stream(frames, use_graph=False), want_frames, "eager stream, cycle %d" % k)
            assert S.stream_mode()[0] == 0

            # batch graph: its own scratch, tables and executable
            din, dout = S.DeviceBuffer.from_numpy(frames[:2]), S.DeviceBuffer(frames[:2].nbytes * 4)
            st, gh = S.Stream(), C.c_void_p()
            try:
                S.check(L.srcnn_batch_graph_create(din.ptr, 40, 24, 2, dout.ptr, st.handle, C.byref(gh)))
                for rep in range(2):
                    S.check(L.srcnn_memset_dev(dout.ptr, 0, dout.nbytes, st.handle))
                    S.check(L.srcnn_batch_graph_launch(gh))
                    st.sync()
                    assert_bit_equal(dout.to_numpy(np.float32, (2, 48, 80)), want_frames[:2], "batch graph launch %d, cycle %d" % (rep, k))
                S.check(L.srcnn_batch_graph_destroy(gh))
            finally:
                st.destroy()
            din.free(); dout.free()

            # ProcessSRCNN surface: a lane with its staging (pageable buffers), then the caller's page-locked buffers in place
            got_rgb, got_conv = S.process_u8(img)
            assert np.array_equal(got_rgb, want_rgb) and np.array_equal(got_conv, want_conv), k
            pin_in, pin_out, pin_conv = S.PinnedArray(img.shape), S.PinnedArray(want_rgb.shape), S.PinnedArray(want_conv.shape)
            try:
                pin_in.array[...] = img
                pin_out.array[...] = 0
                pin_conv.array[...] = 0
                S.check(L.srcnn_process_u8(pin_in.array.ctypes.data, 90, 70, 4, 2.0, 2, pin_out.array.ctypes.data, pin_conv.array.ctypes.data))
                assert np.array_equal(pin_out.array, want_rgb) and np.array_equal(pin_conv.array, want_conv), k
            finally:
                pin_in.free(); pin_out.free(); pin_conv.free()

            # node-level tiled frame: the node lanes of both contexts
            h, w = tall.shape
            din, dout = S.DeviceBuffer.from_numpy(tall), S.DeviceBuffer(tall.nbytes * 4)
            S.check(L.srcnn_y_upscale2x_f32_node_dev(din.ptr, w, h, dout.ptr, 2))
            S.sync()
            assert_bit_equal(dout.to_numpy(np.float32, (2 * h, 2 * w)), want_tall, "node-level frame, cycle %d" % k)
            din.free(); dout.free()

            # stage timers: the event pool and the recorded spans (host-call buffers and bounce slots on the way)
            S.profile_reset()
            S.profile_enable(True)
            try:
                for _ in range(3):
                    assert_bit_equal(S.y_upscale2x(y), want_y, "timed call, cycle %d" % k)
            finally:
                S.profile_enable(False)
            prof = S.profile_read()
            assert [prof[s][1] for s in S.STAGES] == [3, 3, 3], prof
            assert all(prof[s][0] > 0 for s in S.STAGES), prof

            S.check(L.srcnn_trim())
            on_a_fresh_stream("stream call after srcnn_trim, cycle %d" % k)
            assert_bit_equal(S.y_upscale2x(y), want_y, "host call after srcnn_trim, cycle %d" % k)
    finally:
        S.shutdown()
        S.init(0)
