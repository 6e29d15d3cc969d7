// json_mini.hpp — the handful of Json::Value operations the processors' serialize()/deserialize() use
// (reference: JsonCpp, include/infra/processor.hpp:6,93-96).  Only what the hot-path nodes touch: objects of
// bool / int / double / string members, and arrays of values or of objects (the equalizer's bands, the multiband compressor's).  Not a JSON parser: project files are the editor's
// business (out of scope).
#pragma once
#include <map>
#include <string>
#include <variant>
#include <vector>

namespace Json
{
	enum ValueType { nullValue = 0, arrayValue = 6, objectValue = 7 };  // JsonCpp's numbering; only what Value(ValueType) is called with

	class Value
	{
		std::variant<std::monostate, bool, int, double, std::string> scalar;
		std::map<std::string, Value> members;
		std::vector<Value> items;
		bool array = false;

	  public:

		Value() = default;
		Value(bool v) : scalar(v) {}
		Value(int v) : scalar(v) {}
		Value(double v) : scalar(v) {}
		Value(float v) : scalar(static_cast<double>(v)) {}
		Value(const char* v) : scalar(std::string(v)) {}
		Value(std::string v) : scalar(std::move(v)) {}
		Value(ValueType type) : array(type == arrayValue) {}

		// JsonCpp's array operations: append to an array (a null value becomes one), element by index, size() of an array
		bool isArray() const { return array; }
		// an object: what is neither an array nor a scalar.  An object without members and a null value are one here (JsonCpp tells them apart)
		bool isObject() const { return !array && std::holds_alternative<std::monostate>(scalar); }
		Value& append(const Value& v)
		{
			array = true;
			items.push_back(v);
			return items.back();
		}
		Value& operator[](int index)
		{
			// JsonCpp: an index past the end grows the array with null values
			array = true;
			if ((size_t)index >= items.size()) items.resize((size_t)index + 1);
			return items[(size_t)index];
		}
		const Value& operator[](int index) const
		{
			static const Value null_value;
			return index >= 0 && (size_t)index < items.size() ? items[(size_t)index] : null_value;
		}

		Value& operator[](const std::string& key) { return members[key]; }
		const Value& operator[](const std::string& key) const
		{
			static const Value null_value;
			const auto it = members.find(key);
			return it == members.end() ? null_value : it->second;
		}
		bool isMember(const std::string& key) const { return members.count(key) != 0; }
		bool isNull() const { return std::holds_alternative<std::monostate>(scalar) && members.empty() && !array; }
		bool isBool() const { return std::holds_alternative<bool>(scalar); }
		bool isInt() const { return std::holds_alternative<int>(scalar); }
		bool isString() const { return std::holds_alternative<std::string>(scalar); }
		std::string asString() const { return isString() ? std::get<std::string>(scalar) : std::string(); }
		// JsonCpp: isDouble() is true for every numeric value
		bool isDouble() const { return std::holds_alternative<double>(scalar) || std::holds_alternative<int>(scalar); }
		bool asBool() const { return isBool() ? std::get<bool>(scalar) : asDouble() != 0.0; }
		int asInt() const { return static_cast<int>(asDouble()); }
		float asFloat() const { return static_cast<float>(asDouble()); }
		double asDouble() const
		{
			if (std::holds_alternative<double>(scalar)) return std::get<double>(scalar);
			if (std::holds_alternative<int>(scalar)) return std::get<int>(scalar);
			if (std::holds_alternative<bool>(scalar)) return std::get<bool>(scalar) ? 1.0 : 0.0;
			return 0.0;
		}
		size_t size() const { return array ? items.size() : members.size(); }
		// JsonCpp: Value::Members = std::vector<std::string>, in key order
		std::vector<std::string> getMemberNames() const
		{
			std::vector<std::string> names;
			for (const auto& kv : members) names.push_back(kv.first);
			return names;
		}
	};
}
