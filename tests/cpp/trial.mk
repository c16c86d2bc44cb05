# The planner of the trial snapshot (rust-lp_amd/csrc/relp_trial.hpp, plain C++17): plain g++, no library, no GPU.
# `make -C tests/cpp -f trial.mk`
#   test_trial       offsets, overlap, the unit prefix sums, both directions, the refusals, a byte-for-byte model of the copy
#   test_trial_asan  the same program with -fsanitize=address,undefined (a stand-alone program: no preload)
CXX ?= g++
ROOT := ../..
CSRC := $(ROOT)/rust-lp_amd/csrc
DEPS := test_trial.cpp $(CSRC)/relp_trial.hpp

all: test_trial test_trial_asan

test_trial: $(DEPS)
	$(CXX) -std=c++17 -O1 -Wall -Wextra -I$(CSRC) test_trial.cpp -o $@

test_trial_asan: $(DEPS)
	$(CXX) -std=c++17 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -I$(CSRC) test_trial.cpp -o $@

clean:
	rm -f test_trial test_trial_asan
