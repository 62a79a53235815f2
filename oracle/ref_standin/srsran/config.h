/* ORACLE PINNING HARNESS -- TEST INFRASTRUCTURE ONLY.
 *
 * Stand-in for the one third-party header the reference's sections_part3 cell-map sources
 * (drs.cpp, pcc.cpp, pdc.cpp, beamforming_and_antenna_port_mapping.cpp) reach, through
 * dectnrp/common/complex.hpp, and only for the complex sample type. This is the project's own
 * text, not srsRAN's: it holds that one typedef and nothing else. It is on the include path of
 * oracle/Makefile's `ref` target only, so that those four files compile unmodified into
 * oracle/_ref/; neither the oracle nor the product library ever sees it.
 */
#ifndef DNRP_ORACLE_REF_STANDIN_SRSRAN_CONFIG_H
#define DNRP_ORACLE_REF_STANDIN_SRSRAN_CONFIG_H

typedef float _Complex cf_t;

#endif
