# The host side of the column pool (rust-lp_amd/csrc/relp_pool.hpp, plain C++17): plain g++, no library, no GPU.
# `make -C tests/cpp -f pool.mk`
#   test_pool       the sliced-ELL packer, the segment arithmetic of relp_pool_price, the stale rule, the argument checks
#   test_pool_asan  the same program with -fsanitize=address,undefined (a stand-alone program: no preload)
CXX ?= g++
ROOT := ../..
CSRC := $(ROOT)/rust-lp_amd/csrc
DEPS := test_pool.cpp $(CSRC)/relp_pool.hpp

all: test_pool test_pool_asan

test_pool: $(DEPS)
	$(CXX) -std=c++17 -O1 -Wall -Wextra -I$(CSRC) test_pool.cpp -o $@

test_pool_asan: $(DEPS)
	$(CXX) -std=c++17 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -I$(CSRC) test_pool.cpp -o $@

clean:
	rm -f test_pool test_pool_asan
