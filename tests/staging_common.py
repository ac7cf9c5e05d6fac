"""What the tests of the staging layer (bow_amd/csrc/dev_cols.cpp) share: caller buffers at odd byte addresses."""
from bow_amd import capi


class Shifted(capi.DeviceBuffer):
    """`shift` bytes into a device buffer: a device pointer at an odd byte address"""

    def __init__(self, base, shift):
        self.base, self.ptr, self.nbytes = base, base.ptr + shift, base.nbytes - shift

    def free(self):
        self.ptr = None
