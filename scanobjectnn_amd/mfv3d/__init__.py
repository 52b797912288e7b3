"""3DmFV-Net (the reference's `3DmFV-Net/` family; a Python package name cannot start with a digit): the 3DmFV
representation and the k^3 convolutions of its inception trunk on libpcops (csrc/mfv.hip), everything else on the layers the
other families already use."""
