// regenie-amd, the C++ host driver (see driver.h): the pure part of `--step 2 --compute-corr` (driver_ld.cpp), which variant takes which
// column of the LD matrix (check_in_map_from_files / check_ld_list, Geno.cpp:1343-1380, :1443-1453).
#pragma once
#include "driver.h"

namespace rgdrv {

struct LdColumns {
  std::vector<std::string> col_ids;         // the ID of every column
  std::vector<int32_t> col_of_variant;      // per variant of the genotype file: its column, -1: none
  std::vector<uint8_t> absent;              // per column: 1 = forced in, the genotype file has no such variant (a zero column)
  std::vector<int64_t> present;             // the variants that take a column, in file order
};

// forced == nullptr: the variants in file order, a repeated ID takes one column (its first variant's).  Otherwise (--extract
// --forcein-vars) `forced` holds the first token of every line of the extract file: the columns are these IDs in order, a trailing '\r'
// dropped and duplicates ignored, IDs the genotype file does not have included; a second variant with a placed ID is skipped (Geno.cpp:590-593).
inline LdColumns plan_ld_columns(const std::vector<std::string>& snp_ids, const std::vector<std::string>* forced) {
  LdColumns lc;
  lc.col_of_variant.assign(snp_ids.size(), -1);
  std::unordered_map<std::string, int32_t> order;
  if (forced) {
    for (std::string id : *forced) {
      if (!id.empty() && id.back() == '\r') id.pop_back();
      if (order.emplace(id, (int32_t)lc.col_ids.size()).second) lc.col_ids.push_back(id);
    }
    lc.absent.assign(lc.col_ids.size(), 1);
    for (size_t j = 0; j < snp_ids.size(); ++j) {
      auto it = order.find(snp_ids[j]);
      if (it == order.end() || !lc.absent[it->second]) continue;
      lc.col_of_variant[j] = it->second;
      lc.absent[it->second] = 0;
    }
  } else {
    for (size_t j = 0; j < snp_ids.size(); ++j) {
      if (!order.emplace(snp_ids[j], (int32_t)lc.col_ids.size()).second) continue;
      lc.col_of_variant[j] = (int32_t)lc.col_ids.size();
      lc.col_ids.push_back(snp_ids[j]);
    }
    lc.absent.assign(lc.col_ids.size(), 0);
  }
  for (size_t j = 0; j < snp_ids.size(); ++j) if (lc.col_of_variant[j] >= 0) lc.present.push_back((int64_t)j);
  return lc;
}

}  // namespace rgdrv
