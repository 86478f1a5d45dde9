"""``vsrlab.optical_flow.models.raft``: RAFT-small (reference ``src/optical_flow/models/raft/``) with the correlation lookup
on the HIP path (``csrc/raft_corr.hip``).  The encoders, the ConvGRU, the motion encoder and the flow head are library
convolutions; ``corr.correlation`` is the one operation nothing in torch fuses."""
