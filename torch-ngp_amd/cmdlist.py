"""Native command list (csrc/cmdlist.cpp, include/ngp_hip.h ngp_cmdlist_*): the stream operations a chain of library entries issued,
recorded once and replayed from C with no Python between the launches.  graph.GraphedTrainStep records one beside every rest graph it
captures and replays it in the graph's place; the graph stays: it owns the memory pool the recorded pointers live in.
"""
import ctypes

import _ngp_capi as capi


class CommandList:
    def __init__(self):
        h = ctypes.c_void_p()
        capi.check(capi.lib.ngp_cmdlist_create(ctypes.byref(h)))
        self.handle = h.value

    # `with cl:` records what the library's entries issue on this thread inside the block; an exception leaves the list closed and unusable
    def __enter__(self):
        capi.check(capi.lib.ngp_cmdlist_begin(self.handle))
        return self

    def __exit__(self, exc_type, exc, tb):
        capi.check(capi.lib.ngp_cmdlist_end(self.handle))
        return False

    def count(self):
        n = ctypes.c_uint32()
        capi.check(capi.lib.ngp_cmdlist_count(self.handle, ctypes.byref(n)))
        return n.value

    def names(self):
        """the entries by name, in order: kernel symbols, 'memset', 'memcpy'"""
        buf = ctypes.create_string_buffer(512)
        out = []
        for i in range(self.count()):
            capi.check(capi.lib.ngp_cmdlist_entry_name(self.handle, i, buf, len(buf)))
            out.append(buf.value.decode())
        return out

    def mark(self, mark_id, after=-1):
        capi.check(capi.lib.ngp_cmdlist_mark(self.handle, mark_id, after))

    def replay(self, stream):
        capi.check(capi.lib.ngp_cmdlist_replay(self.handle, stream))

    def wait_mark(self, mark_id, stream):
        capi.check(capi.lib.ngp_cmdlist_wait_mark(self.handle, mark_id, stream))

    def destroy(self):
        if self.handle is not None:
            h, self.handle = self.handle, None
            capi.check(capi.lib.ngp_cmdlist_destroy(h))

    def __del__(self):
        try:
            self.destroy()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass
