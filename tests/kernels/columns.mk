# The kernel harness of the columns added in place (test infrastructure): one extern "C" entry that runs relp::launch_tab_add_columns
# of the shipped librelp_engine.so on device images a test constructs (tests/kernel_harness_columns.py).
# `make -C tests/kernels -f columns.mk`
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
ROOT := ../..
CSRC := $(ROOT)/rust-lp_amd/csrc

all: librelp_kernel_harness_columns.so

librelp_kernel_harness_columns.so: harness_columns.cpp $(CSRC)/relp_kernels.h $(CSRC)/relp_layout.hpp $(ROOT)/rust-lp_amd/librelp_engine.so
	$(HIPCC) --offload-arch=$(ARCH) -O2 -std=c++17 -fPIC -Wall -Wextra -x hip -shared -I$(CSRC) -I$(ROOT)/include $< -o $@ \
	    -L$(ROOT)/rust-lp_amd -lrelp_engine -Wl,-rpath,'$$ORIGIN/../../rust-lp_amd'

clean:
	rm -f librelp_kernel_harness_columns.so
