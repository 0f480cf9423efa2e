"""Test-only stand-in for DINO's ``util.misc``: the detection backbone file imports ``NestedTensor`` from it and only stores
``tensors`` / ``mask`` on it."""


class NestedTensor(object):
    def __init__(self, tensors, mask):
        self.tensors = tensors
        self.mask = mask
