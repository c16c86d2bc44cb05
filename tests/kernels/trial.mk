# The kernel harness of the trial snapshot (test infrastructure): one extern "C" entry that runs relp::launch_tab_trial_copy of the
# shipped librelp_engine.so on a device image a test constructs (tests/kernel_harness_trial.py).  `make -C tests/kernels -f trial.mk`
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
ROOT := ../..
CSRC := $(ROOT)/rust-lp_amd/csrc

all: librelp_kernel_harness_trial.so

librelp_kernel_harness_trial.so: harness_trial.cpp $(CSRC)/relp_kernels.h $(CSRC)/relp_trial.hpp $(ROOT)/rust-lp_amd/librelp_engine.so
	$(HIPCC) --offload-arch=$(ARCH) -O2 -std=c++17 -fPIC -Wall -Wextra -x hip -shared -I$(CSRC) -I$(ROOT)/include $< -o $@ \
	    -L$(ROOT)/rust-lp_amd -lrelp_engine -Wl,-rpath,'$$ORIGIN/../../rust-lp_amd'

clean:
	rm -f librelp_kernel_harness_trial.so
