"""Label capacities of the linear classifier: the one definition, imported by
the driver (models/classifier.py) and by the kernel bindings (ops/hip.py).
csrc/server/jubaclassifier.cpp kLabelCaps is the native twin."""

# capacities the tables grow through
LABEL_CAPS = (8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384)
# up to here the LC-templated kernels of csrc/hip/linear.hip run (jb_linear.hpp
# kTemplateMaxLC); above it the label-chunked ones (csrc/hip/linear_chunked.hip),
# which take any multiple of CHUNK_LABELS. Growing the tables to a capacity
# above it is checked against the free memory first.
TEMPLATE_MAX_LC = 1024
CHUNK_LABELS = 256
