# The kernel harness of the Gomory cuts (test infrastructure): one extern "C" entry that runs relp::launch_tab_gomory of the shipped
# librelp_engine.so on device images a test constructs (tests/kernel_harness_gomory.py).  `make -C tests/kernels -f gomory.mk`
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
ROOT := ../..
CSRC := $(ROOT)/rust-lp_amd/csrc

all: librelp_kernel_harness_gomory.so

librelp_kernel_harness_gomory.so: harness_gomory.cpp $(CSRC)/relp_kernels.h $(ROOT)/rust-lp_amd/librelp_engine.so
	$(HIPCC) --offload-arch=$(ARCH) -O2 -std=c++17 -fPIC -Wall -Wextra -x hip -shared -I$(CSRC) -I$(ROOT)/include $< -o $@ \
	    -L$(ROOT)/rust-lp_amd -lrelp_engine -Wl,-rpath,'$$ORIGIN/../../rust-lp_amd'

clean:
	rm -f librelp_kernel_harness_gomory.so
