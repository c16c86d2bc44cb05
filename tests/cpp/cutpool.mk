# The host side of the cut pool (rust-lp_amd/csrc/relp_cutpool.hpp over relp_pool.hpp, plain C++17): plain g++, no library, no GPU.
# `make -C tests/cpp -f cutpool.mk`
#   test_cutpool       the adapter onto the sliced-ELL packer, the norms, the segment arithmetic, the key, the argument checks
#   test_cutpool_asan  the same program with -fsanitize=address,undefined (a stand-alone program: no preload)
CXX ?= g++
ROOT := ../..
CSRC := $(ROOT)/rust-lp_amd/csrc
DEPS := test_cutpool.cpp $(CSRC)/relp_cutpool.hpp $(CSRC)/relp_pool.hpp

all: test_cutpool test_cutpool_asan

test_cutpool: $(DEPS)
	$(CXX) -std=c++17 -O1 -Wall -Wextra -I$(CSRC) test_cutpool.cpp -o $@

test_cutpool_asan: $(DEPS)
	$(CXX) -std=c++17 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -I$(CSRC) test_cutpool.cpp -o $@

clean:
	rm -f test_cutpool test_cutpool_asan
